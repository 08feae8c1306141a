"""Early-stopped Sinkhorn solves (nits < L) on every kernel family, held to the float64 stopped_sweep of
tests/test_sinkhorn_early_stop_cpu.py.  The inputs and the conditions that make the count a property of the inputs are
asserted there; here L = 40, Lmin = 3, eps = 0.5 and thresh = 1e-2 (one launch, weighted n = 1024, places its thresh: see
stop_thresh), the stop falls at iterations 4 to 12, and the problems of one launch stop at different counts.

Size and options -> kernel, read from the dispatch code (file:line of the rule):

  register path, n <= 128 (kccotgan_amd/csrc/sinkhorn.hip: sink_geom :1262-1281 -- lanes per line :1270, option
  sinkhorn_lanes_per_line at 32 < n <= 64 :1271-1276, entries per lane :1277-1278; the <EPT,LPR> switch KCCOT_SK_DISPATCH
  :1309-1323; forward: sinkhorn_shortcut = 1 -> sinkhorn_fwd_reg :1362 / sinkhorn_fwd_reg_w :1355, 0 -> sinkhorn_fwd_reg_full
  :1364 / sinkhorn_fwd_reg_full_w :1357; backward sinkhorn_bwd_reg :1421, sinkhorn_bwd_reg_w :1418, sinkhorn_bwd_reg_dw :1414)
    n      sinkhorn_lanes_per_line   forward <EPT,LPR>   backward <EPT,LPR>
    7      0                         <1,16>              <1,16>
    24     0                         <2,16>              <2,16>
    48     0                         <8,8>               <4,16>
    48     4                         <16,4>              <16,4>
    48     8                         <8,8>               <8,8>
    48     16                        <4,16>              <4,16>
    64     0                         <8,8>               <4,16>
    128    0                         <16,8>              <16,8>
  every row runs unweighted (2.1) and weighted (2.4), each with sinkhorn_shortcut = 1 and 0.

  streaming path, 128 < n <= 1024 (kccotgan_amd/csrc/sinkhorn_gen.hip: launch_sinkhorn_fwd_gen :611-640, wide = n % 4 == 0
  and C 16-byte aligned :627; launch_sinkhorn_bwd_gen :642-664); unweighted solves reach it under sinkhorn_coop = 0 (:618,
  :648; sinkhorn_coop.hip:470, :507), weighted and conditional solves always (:617-618)
    n            C aligned          forward kernel, unweighted / weighted                    rule
    131          yes                sinkhorn_fwd_gen<false> / <true>                          n % 4 != 0            :635 / :629
    132          no (4 bytes off)   sinkhorn_fwd_gen<false> / <true>                          (uintptr_t)C % 16     :627
    132 (cond.)  yes                sinkhorn_fwd_gen16<4,true>                                n <= 256              :630
    256          yes                sinkhorn_fwd_gen16<4,false> / <4,true>                    n <= 256              :636 / :630
    260          yes                sinkhorn_fwd_gen16<8,false> / <8,true>                    n <= 512              :637 / :631
    516, 1024    yes                sinkhorn_fwd_gen4<4,false> / <4,true>                     n <= 1024             :638 / :632
  backward at every such n: sinkhorn_bwd_gen<false> :660, sinkhorn_bwd_gen<true> (_bwd_f32, conditional _bwd_f32) :659,
  sinkhorn_bwd_gen<true,true> (_bwd_dw_f32, conditional _bwd_dw_f32) :658.

  multi-CU path, unweighted, default options (kccotgan_amd/csrc/sinkhorn_coop.hip: sinkhorn_coop_eligible :505-508,
  launch_sinkhorn_fwd_coop :570-585 and launch_sinkhorn_bwd_coop :587-605, ept = ceil(n / 64) :577 / :593, the switch :582 /
  :598; the per-XCD layout ll_xcd_map :549-555, grid :580 / :596)
    n            kernels                               layout
    131, 256     sinkhorn_fwd_ll<4>, sinkhorn_bwd_ll<4>    per XCD (nprob <= 8, n <= 256); 2-D grid under sinkhorn_coop_xcd = 0
    260          sinkhorn_fwd_ll<8>, sinkhorn_bwd_ll<8>    2-D grid
    516, 1024    sinkhorn_fwd_ll<16>, sinkhorn_bwd_ll<16>  2-D grid, nprob = 2 (three problems of 64 workgroups sit on the
                                                           co-residency cap)

  conditional mode (w_div = 2; Q = 2 weight rows on the shared C3): n = 48 the register kernels <8,8> / <4,16>
  (sinkhorn_fwd_reg_w, sinkhorn_bwd_reg_w, sinkhorn_bwd_reg_dw), n = 132 and 260 the streaming kernels of the table above.

  fused launches, n <= 64 (sinkhorn.hip: kccot_sinkhorn_fused_eligible / _roles_eligible :1451-1471): n = 24 and 48, three
  problems through kccot_sinkhorn_divergence_fused_f32, four through kccot_mixed_sinkhorn_loss_fwd_f32 with
  KCCOT_MIXED_CMIX_GIVEN; sinkhorn_fused_roles = 1 -> sinkhorn_fused_roles, 0 -> sinkhorn_fused_reg; sinkhorn_shortcut 1 and 0.

What every case asserts, k[p] being the float64 count of problem p:
  1. nits_out[p] == k[p], no slack; nits_out[nprob + p] <= k[p], with equality where no jump can happen (streaming and
     multi-CU kernels, sinkhorn_shortcut = 0).
  2. The same bits as the exact-length run: problem p alone with L = Lmin = k[p], where the stop rule plays no part -- cost,
     pi_out, dC, da, db and history rows [0, k) of u and v.  (Conditional mode: cost and history against the weighted entry
     point on the same matrix and weights; the fused launches: cost and dC of problem p in a launch with L = Lmin = k[p].)
  3. Against float64 stopped_sweep with the project's existing bounds: cost relative 2e-5 and dC atol 2e-4 max|ref|
     (tests/test_gpu_parity.py:338-340), the loss of a combination of costs relative 1e-4 (:1423); final duals, da, db (dw,
     domega): |got - ref| <= 4 max(yard, 2^-24) max|ref| with yard the float32 run of stopped_sweep against its float64 run,
     per quantity over the problems of a launch (the rule of tests/test_gpu_weight_grad.py:solver_yardstick; it measures the
     reference, never the kernel; taken problem by problem instead, one case on the MI355X -- n = 7, unweighted, v after 7
     iterations: error 3.35e-7 where the float32 reference happens to be within 8.2e-8 -- sits at 4.09 yardsticks).  The
     register kernels' history is in log2 units and is converted in float64 first (dual_unit).  Error, yardstick and ratio
     are printed before each assertion (-s); DESIGN.md records the worst figure per instantiation.
  4. History rows at and beyond k are never read: the backward is run again with those rows overwritten by +inf and gives
     the same dC, da and db bits.  (It is also printed whether the forward left them at their NaN fill.)

Every test reads its options on entry and fails unless they are at their defaults; options are set through L.options(...) only.
Every buffer handed to the C ABI lies between NaN-filled guard zones and workspaces are exactly as long as the queries say.
"""
import functools
import math

import pytest
import torch

import test_gpu_conditional_sinkhorn as GC
import test_gpu_weight_grad as GD
import test_sinkhorn_early_stop_cpu as E
from test_gpu_weighted_sinkhorn import Buf, OffsetBuf, workspace, call, same_bits, within, rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64 = torch.float64
F32 = torch.float32
I32 = torch.int32
DEFAULTS = {"sinkhorn_shortcut": 1, "sinkhorn_coop": 1, "sinkhorn_coop_xcd": 1, "sinkhorn_lanes_per_line": 0, "sinkhorn_fused": 1,
            "sinkhorn_fused_roles": 1}
STOP_COUNT, STOP_INDEX = 0, 1
GCOST = (1.0, -0.5, 2.0)                  # upstream gradient of problem p of stop_problems(n), wherever it sits in a launch
COST_RTOL, DC_ATOL = 2e-5, 2e-4           # tests/test_gpu_parity.py:338-340
LOSS_RTOL = 1e-4                          # the loss of a combination of costs: tests/test_gpu_parity.py:1423, DESIGN.md section 3
EPS, LIT, LMIN = E.STOP_EPS, E.STOP_L, E.STOP_LMIN
INF = float("inf")


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    assert (_lib.STOP_COUNT, _lib.STOP_INDEX) == (STOP_COUNT, STOP_INDEX)
    return _lib


def at_defaults(L):
    got = {k: L.get_option(k) for k in DEFAULTS}
    assert got == DEFAULTS, "options not at their defaults on entry: %s" % got


# ================================================================ the harness
def poison_rows_past(bufs, counts):
    """Overwrite history rows [k, L) of every problem with +inf; returns whether the forward had left them all at the NaN fill."""
    untouched = True
    for key in ("u", "v"):
        h = bufs[key].t.view(len(counts), -1, bufs[key].t.shape[-1])
        for p, k in enumerate(counts):
            untouched &= bool(torch.isnan(h[p, k:]).all())
            h[p, k:] = INF
    return untouched


def solve(L, C, a, b, eps, Lit, Lmin, thresh, stop_mode=STOP_COUNT, gcost=GCOST, c_off=0, again=None):
    """One launch through the C ABI: forward (with pi_out), backward, and the backward once more with the history rows past the
    count overwritten by +inf (check 4).  a = b = None: kccot_sinkhorn_fwd_f32 / _bwd_f32 (dC); otherwise the weighted entry
    points, _bwd_f32 (dC0) and _bwd_dw_f32 (dC, da, db).  again = (L2, Lmin2): the forward is then launched a second time on
    the SAME buffers and workspace; its cost and counts come back as cost2 / nits2."""
    nprob, n, _ = C.shape
    Lh = max(Lit, 1)
    weighted = a is not None
    bufs = {"C": OffsetBuf(C.shape, C, c_off), "u": Buf((nprob, Lh, n)), "v": Buf((nprob, Lh, n)), "cost": Buf((nprob,)),
            "nits": Buf((2 * nprob,), dtype=I32), "pi": Buf(C.shape), "dC": Buf(C.shape),
            "g": Buf((nprob,), torch.tensor(gcost[:nprob]))}
    if weighted:
        bufs.update({"a": Buf(a.shape, a), "b": Buf(b.shape, b), "dC0": Buf(C.shape), "da": Buf((nprob, n)), "db": Buf((nprob, n))})
    ws, wsb = workspace(L.lib.kccot_sinkhorn_workspace_bytes(nprob, n))
    bufs["ws"] = ws
    wp = ws.ptr() if wsb else None
    P = {k: bf.ptr() for k, bf in bufs.items()}

    def forward(Lit_, Lmin_):
        if weighted:
            call(L, "kccot_sinkhorn_weighted_fwd_f32", P["C"], P["a"], P["b"], nprob, n, eps, Lit_, Lmin_, thresh, stop_mode, P["u"],
                 P["v"], P["cost"], P["nits"], P["pi"], wp, wsb, None)
        else:
            call(L, "kccot_sinkhorn_fwd_f32", P["C"], nprob, n, eps, Lit_, Lmin_, thresh, stop_mode, P["u"], P["v"], P["cost"],
                 P["nits"], P["pi"], wp, wsb, None)

    def backward():
        if weighted:
            call(L, "kccot_sinkhorn_weighted_bwd_f32", P["C"], P["a"], P["b"], P["u"], P["v"], P["nits"], nprob, n, eps, Lh, P["g"],
                 P["dC0"], wp, wsb, None)
            call(L, "kccot_sinkhorn_weighted_bwd_dw_f32", P["C"], P["a"], P["b"], P["u"], P["v"], P["nits"], nprob, n, eps, Lh,
                 P["g"], P["dC"], P["da"], P["db"], wp, wsb, None)
        else:
            call(L, "kccot_sinkhorn_bwd_f32", P["C"], P["u"], P["v"], P["nits"], nprob, n, eps, Lh, P["g"], P["dC"], wp, wsb, None)
        return {k: bufs[k].t.clone() for k in (("dC0", "dC", "da", "db") if weighted else ("dC",))}

    forward(Lit, Lmin)
    out = {k: bufs[k].t.clone() for k in ("cost", "pi", "u", "v")}
    flat = bufs["nits"].t.tolist()
    out["nits"], out["executed"] = flat[:nprob], flat[nprob:]
    # a NaN cost or a negative count: the solver aborted.  That fails the test; nothing is tried again.
    assert bool(torch.isfinite(out["cost"]).all()) and all(0 < k <= Lit for k in out["nits"]), (out["cost"], flat)
    out.update(backward())
    out["rows_past_k_untouched"] = poison_rows_past(bufs, out["nits"])
    for k, x in backward().items():
        assert same_bits(x, out[k]), "%s changes when the history rows at and beyond the count are overwritten (n=%d)" % (k, n)
    if again is not None:
        forward(*again)
        out["cost2"], out["nits2"] = bufs["cost"].t.clone(), bufs["nits"].t.tolist()
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d)" % (k, n)
    return out


def launch_inputs(n, kind, idx):
    C, _, _, _ = E.stop_problems(n)
    sel = list(idx)
    if kind == "uniform":
        return C[sel].contiguous(), None, None
    a, b = E.weights_of(n, kind)
    return C[sel].contiguous(), a[sel].contiguous(), b[sel].contiguous()


def two_with_different_counts(n, kind):
    ks = E.references(n, kind, GCOST)[1]
    return next((i, j) for i in range(3) for j in range(i + 1, 3) if ks[i] != ks[j])


def dual_unit(n):
    """What one unit of a history entry is worth: the register kernels (n <= 128) carry and store the duals in log2 units,
    U = u / (eps ln 2) (kccotgan_amd/csrc/sinkhorn.hip:18, :181, :543), the streaming and multi-CU kernels in natural units
    (sinkhorn_gen.hip:171, sinkhorn_coop.hip:281).  Exact in float64; the comparison is made there."""
    return EPS * math.log(2.0) if n <= 128 else 1.0


def against_fp64(tag, out, r64, r32, ks):
    """Check 3 for a launch: r64 / r32 are stopped_sweep's float64 / float32 results of its problems, in launch order.  Cost
    and dC problem by problem; the final duals, da and db per quantity over the problems of the launch, error and yardstick
    both relative to the largest reference entry of the launch, as tests/test_gpu_weight_grad.py:solver_yardstick takes them.
    Returns the worst error as a fraction of its bound."""
    ratios = []
    for pos, k in enumerate(ks):
        cost_err = abs(float(out["cost"][pos]) - float(r64[pos][0])) / abs(float(r64[pos][0]))
        dC_err = rel_err(out["dC"][pos], r64[pos][2])
        print("%-44s cost err %.3e (bound %g)  dC err %.3e (bound %g)" % ("%s p[%d] k=%d" % (tag, pos, k), cost_err, COST_RTOL, dC_err,
                                                                        DC_ATOL))
        assert cost_err <= COST_RTOL, (tag, pos, cost_err)
        assert bool(torch.isfinite(out["dC"][pos]).all()) and dC_err <= DC_ATOL, (tag, pos, dC_err)
        ratios += [cost_err / COST_RTOL, dC_err / DC_ATOL]
    unit = dual_unit(out["u"].shape[-1])
    last = {key: torch.stack([out[key][pos, k - 1] for pos, k in enumerate(ks)]).double().cpu() * unit for key in ("u", "v")}
    pairs = [("u[k-1]", last["u"], 5), ("v[k-1]", last["v"], 6)]
    if "da" in out:
        pairs += [("da", out["da"], 3), ("db", out["db"], 4)]
    for name, got, i in pairs:
        ref, f32 = torch.stack([r[i] for r in r64]), torch.stack([r[i] for r in r32])
        ratios.append(within("%s %s" % (tag, name), got, ref, rel_err(f32, ref)) / 4.0)
    return max(ratios)


def check(L, tag, n, kind, idx=(0, 1, 2), c_off=0, jump_possible=False, again=False, Lit=LIT, Lmin=LMIN, mode=STOP_COUNT,
          exact_length=True, **opts):
    """Checks 1 to 4 for the problems `idx` of stop_problems(n) with the marginals `kind`, under the options `opts`."""
    C, a, b = launch_inputs(n, kind, idx)
    thresh = E.stop_thresh(n, kind)
    gcost = tuple(GCOST[p] for p in idx)
    index = mode == STOP_INDEX
    r64 = list(zip(*E.references(n, kind, GCOST, Lmin, Lit, index)))
    r32 = list(zip(*E.references(n, kind, GCOST, Lmin, Lit, index, F32)))
    ks = [r64[p][1] for p in idx]
    with L.options(**opts):
        out = solve(L, C, a, b, EPS, Lit, Lmin, thresh, mode, gcost, c_off, again=(5, 5) if again else None)
        print("%s n=%d %s thresh=%.4g: float64 counts %s, device %s, executed %s, rows past k left at the NaN fill: %s"
              % (tag, n, kind, thresh, ks, out["nits"], out["executed"], out["rows_past_k_untouched"]))
        assert out["nits"] == ks, (tag, out["nits"], ks)                                           # 1
        if jump_possible:
            assert all(0 < e <= k for e, k in zip(out["executed"], ks)), (tag, out["executed"])
        else:
            assert out["executed"] == ks, (tag, out["executed"], ks)
        if "dC0" in out:
            assert same_bits(out["dC"], out["dC0"]), tag + ": dC of the _dw call differs from kccot_sinkhorn_weighted_bwd_f32"
        if again:
            fresh = solve(L, C, a, b, EPS, 5, 5, thresh, mode, gcost, c_off)
            assert out["nits2"] == [5] * (2 * len(idx)) and fresh["nits"] == [5] * len(idx), (tag, out["nits2"])
            assert same_bits(out["cost2"], fresh["cost"]), tag + ": the launch after an early-stopped one is disturbed"
        for pos, p in enumerate(idx if exact_length else ()):                                      # 2
            k = ks[pos]
            one = solve(L, C[pos:pos + 1].contiguous(), None if a is None else a[pos:pos + 1].contiguous(),
                        None if b is None else b[pos:pos + 1].contiguous(), EPS, k, k, thresh, mode, gcost[pos:pos + 1], c_off)
            assert one["nits"] == [k], (tag, p, one["nits"])
            for key in ("cost", "pi", "dC", "da", "db"):
                if key in out:
                    assert same_bits(one[key][0], out[key][pos]), "%s: %s of problem %d differs from the run with L = Lmin = %d" % (
                        tag, key, p, k)
            for key in ("u", "v"):
                assert same_bits(one[key][0, :k], out[key][pos, :k]), "%s: %s rows [0, %d) of problem %d differ" % (tag, key, k, p)
    worst = against_fp64("%s n=%d" % (tag, n), out, [r64[p] for p in idx], [r32[p] for p in idx], ks)              # 3
    print("WORST %s n=%d %s: %.2f of the bound" % (tag, n, kind, worst))
    return out


# ================================================================ 2.1 / 2.4 the register path, unweighted and weighted
REG = [(7, 0, "<1,16>/<1,16>"), (24, 0, "<2,16>/<2,16>"), (48, 0, "<8,8>/<4,16>"), (48, 4, "<16,4>/<16,4>"), (48, 8, "<8,8>/<8,8>"),
       (48, 16, "<4,16>/<4,16>"), (64, 0, "<8,8>/<4,16>"), (128, 0, "<16,8>/<16,8>")]


@pytest.mark.parametrize("kind", ["uniform", "ab"])
@pytest.mark.parametrize("n,lanes,shapes", REG)
def test_register_path_stops_early(L, n, lanes, shapes, kind):
    """sinkhorn_fwd_reg / _reg_full (uniform) and sinkhorn_fwd_reg_w / _reg_full_w (ab) with their reverse sweeps; the counts and
    every output bit agree between sinkhorn_shortcut = 1 and 0."""
    at_defaults(L)
    runs = {sc: check(L, "reg %s lanes=%d shortcut=%d" % (shapes, lanes, sc), n, kind, jump_possible=bool(sc),
                      sinkhorn_lanes_per_line=lanes, sinkhorn_shortcut=sc) for sc in (1, 0)}
    at_defaults(L)
    assert runs[1]["nits"] == runs[0]["nits"]
    for key in ("cost", "pi", "dC", "da", "db"):
        if key in runs[0]:
            assert same_bits(runs[1][key], runs[0][key]), "%s differs between sinkhorn_shortcut = 1 and 0" % key


# ================================================================ 2.2 / 2.4 the streaming path, unweighted and weighted
STREAM = [(131, 0, "gen"), (132, 1, "gen(C+4B)"), (256, 0, "gen16<4>"), (260, 0, "gen16<8>"), (516, 0, "gen4<4>"), (1024, 0, "gen4<4>")]


@pytest.mark.parametrize("kind", ["uniform", "ab"])
@pytest.mark.parametrize("n,c_off,kernel", STREAM)
def test_streaming_path_stops_early(L, n, c_off, kernel, kind):
    """sinkhorn_fwd_gen* <.., false> with sinkhorn_bwd_gen<false> under sinkhorn_coop = 0; the weighted twins with
    sinkhorn_bwd_gen<true> and <true,true> (weighted work never takes the multi-CU solver; the option is set all the same)."""
    at_defaults(L)
    check(L, "stream %s" % kernel, n, kind, c_off=c_off, sinkhorn_coop=0)
    at_defaults(L)


# ================================================================ 2.3 the multi-CU path
COOP = [(131, 3, 1, "ll<4> per XCD"), (131, 3, 0, "ll<4> 2-D grid"), (256, 3, 1, "ll<4> per XCD"), (256, 3, 0, "ll<4> 2-D grid"),
        (260, 3, 1, "ll<8>"), (516, 2, 1, "ll<16>"), (1024, 2, 1, "ll<16>")]


@pytest.mark.parametrize("n,nprob,xcd,kernel", COOP)
def test_multi_cu_path_stops_early(L, n, nprob, xcd, kernel):
    """The workgroups of the problem that stops first leave while the other problems' go on exchanging; the launch that follows
    on the same buffers and workspace (Lmin = L = 5) must find nothing of it."""
    at_defaults(L)
    idx = (0, 1, 2) if nprob == 3 else two_with_different_counts(n, "uniform")
    out = check(L, "coop %s" % kernel, n, "uniform", idx=idx, again=True, sinkhorn_coop_xcd=xcd)
    assert len(set(out["nits"])) >= 2, out["nits"]
    at_defaults(L)


# ================================================================ 2.5 conditional mode
COND_Q = 2


def cond_solve(L, C3, w, omega, eps, Lit, Lmin, gloss):
    """kccot_sinkhorn_conditional_fwd_f32, _bwd_f32 (dC0) and _bwd_dw_f32 (dC3, dw, domega), then both backwards again with the
    history rows past each count overwritten by +inf."""
    Q, n = w.shape
    bufs = {"C3": Buf(C3.shape, C3), "w": Buf(w.shape, w), "u": Buf((Q, 3, Lit, n)), "v": Buf((Q, 3, Lit, n)), "cost": Buf((Q, 3)),
            "nits": Buf((2, Q, 3), dtype=I32), "loss": Buf((1,)), "dC0": Buf(C3.shape), "dC3": Buf(C3.shape), "dw": Buf((Q, n)),
            "dom": Buf((Q,)), "g": Buf((1,), torch.tensor([gloss]))}
    if omega is not None:
        bufs["omega"] = Buf((Q,), omega)
    op = bufs["omega"].ptr() if omega is not None else None
    ws0, wsb0 = workspace(L.lib.kccot_sinkhorn_conditional_workspace_bytes(Q, n))
    ws, wsb = workspace(L.lib.kccot_sinkhorn_conditional_dw_workspace_bytes(Q, n))
    bufs["ws0"], bufs["ws"] = ws0, ws
    P = {k: bf.ptr() for k, bf in bufs.items()}
    call(L, "kccot_sinkhorn_conditional_fwd_f32", P["C3"], P["w"], op, Q, n, eps, Lit, Lmin, E.THRESH, P["u"], P["v"], P["cost"],
         P["nits"], P["loss"], P["ws0"], wsb0, None)
    out = {k: bufs[k].t.clone() for k in ("cost", "loss", "u", "v")}
    flat = bufs["nits"].t.reshape(-1).tolist()
    out["nits"], out["executed"] = flat[:3 * Q], flat[3 * Q:]
    assert bool(torch.isfinite(out["cost"]).all()) and all(0 < k <= Lit for k in out["nits"]), (out["cost"], flat)

    def backward():
        call(L, "kccot_sinkhorn_conditional_bwd_f32", P["g"], P["C3"], P["w"], op, P["u"], P["v"], P["nits"], Q, n, eps, Lit,
             P["dC0"], P["ws0"], wsb0, None)
        call(L, "kccot_sinkhorn_conditional_bwd_dw_f32", P["g"], P["C3"], P["w"], op, P["u"], P["v"], P["nits"], Q, n, eps, Lit,
             P["dC3"], P["cost"], P["dw"], P["dom"], P["ws"], wsb, None)
        return {k: bufs[k].t.clone() for k in ("dC0", "dC3", "dw", "dom")}

    out.update(backward())
    out["rows_past_k_untouched"] = poison_rows_past(bufs, out["nits"])
    for k, x in backward().items():
        assert same_bits(x, out[k]), "%s changes when the history rows at and beyond the count are overwritten (n=%d)" % (k, n)
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d Q=%d)" % (k, n, Q)
    return out


@functools.lru_cache(maxsize=None)
def cond_pieces(n, dtype):
    """Per (q, k): cost, count, dcost/dC3[k], da + db and the final duals of W(C3[k]; w_q, w_q) at g = 1 by stopped_sweep."""
    C3, w, (eps, Lit, Lmin) = E.cond_problem(n, COND_Q)
    cost, dC, dw = torch.zeros(COND_Q, 3, dtype=dtype), torch.zeros(COND_Q, 3, n, n, dtype=dtype), torch.zeros(COND_Q, 3, n, dtype=dtype)
    ks, duals = [], []
    for q in range(COND_Q):
        for k in range(3):
            r = E.stopped_sweep(C3[k], w[q], w[q], eps, Lit, Lmin, E.THRESH, False, 1.0, dtype)
            cost[q, k], dC[q, k], dw[q, k] = r[0], r[2], r[3] + r[4]
            ks.append(r[1])
            duals.append((r[5], r[6]))
    return cost, dC, dw, ks, duals


@pytest.mark.parametrize("n,kernel", [(48, "reg_w <8,8>/<4,16>"), (132, "gen16<4,true>"), (260, "gen16<8,true>")])
def test_conditional_mode_stops_early(L, n, kernel):
    """Three problems per weight row on the shared C3, Q = 2 rows: six counts in one launch, asserted one by one."""
    at_defaults(L)
    assert E.stop_thresh(n, "cond") == E.THRESH                 # the conditional entry points take thresh, the wrappers 1e-2
    C3, w, (eps, Lit, Lmin) = E.cond_problem(n, COND_Q)
    assert same_bits(w, GC.problem(n)[1][:COND_Q])
    omega = GC.problem(n)[2][:COND_Q]
    p64, p32 = cond_pieces(n, F64), cond_pieces(n, F32)
    ks = p64[3]
    assert p32[3] == ks and len(set(ks)) >= 2
    worst = 0.0
    for om, gl in ((None, 1.0), ((omega / omega.sum()).contiguous(), -0.5)):
        tag = "cond %s n=%d omega=%s gloss=%g" % (kernel, n, "1/Q" if om is None else "given", gl)
        out = cond_solve(L, C3, w, om, eps, Lit, Lmin, gl)
        print("%s: float64 counts %s, device %s, executed %s, rows past k left at the NaN fill: %s"
              % (tag, ks, out["nits"], out["executed"], out["rows_past_k_untouched"]))
        for i, k in enumerate(ks):                                                                 # 1, one by one
            assert out["nits"][i] == k, (tag, "q=%d k=%d" % divmod(i, 3), out["nits"][i], k)
            assert 0 < out["executed"][i] <= k if n <= 128 else out["executed"][i] == k, (tag, i, out["executed"])
        assert same_bits(out["dC3"], out["dC0"]), tag + ": dC3 differs from kccot_sinkhorn_conditional_bwd_f32"
        for i, k in enumerate(ks):                                                                 # 2
            q, k3 = divmod(i, 3)
            one = solve(L, C3[k3:k3 + 1].contiguous(), w[q:q + 1].contiguous(), w[q:q + 1].contiguous(), eps, k, k, E.THRESH,
                        gcost=(1.0,))
            assert one["nits"] == [k]
            assert same_bits(one["cost"][0], out["cost"][q, k3]), "%s: cost of (q=%d, k=%d) differs from L = Lmin = %d" % (tag, q, k3, k)
            for key in ("u", "v"):
                assert same_bits(one[key][0, :k], out[key][q, k3, :k]), "%s: %s rows [0, %d) of (q=%d, k=%d) differ" % (tag, key, k, q, k3)
        for i, k in enumerate(ks):                                                                 # 3
            q, k3 = divmod(i, 3)
            cost_err = abs(float(out["cost"][q, k3]) - float(p64[0][q, k3])) / abs(float(p64[0][q, k3]))
            print("%-44s err %.3e  (bound %g)" % ("%s cost[%d,%d]" % (tag, q, k3), cost_err, COST_RTOL))
            assert cost_err <= COST_RTOL
            worst = max(worst, cost_err / COST_RTOL)
            for key, j in (("u", 0), ("v", 1)):
                r = within("%s %s[k-1] (q=%d, k=%d)" % (tag, key, q, k3), out[key][q, k3, k - 1].double().cpu() * dual_unit(n), p64[4][i][j],
                           rel_err(p32[4][i][j], p64[4][i][j]))
                worst = max(worst, r / 4.0)
        ref_loss, ref_dC = GC.combine64(p64[0], p64[1], om, COND_Q, gl)
        ref_dw, ref_dom = GD.cond_combine((p64[0], p64[2]), om, COND_Q, gl)
        y_dw, y_dom = GD.cond_combine((p32[0], p32[2]), om, COND_Q, gl)
        dC_err = rel_err(out["dC3"], ref_dC)
        print("%-44s err %.3e  (bound %g)" % (tag + " dC3", dC_err, DC_ATOL))
        assert bool(torch.isfinite(out["dC3"]).all()) and dC_err <= DC_ATOL
        loss_err = abs(float(out["loss"]) - float(ref_loss)) / abs(float(ref_loss))
        print("%-44s err %.3e  (bound %g)" % (tag + " loss", loss_err, LOSS_RTOL))
        assert loss_err < LOSS_RTOL
        worst = max(worst, dC_err / DC_ATOL, loss_err / LOSS_RTOL,
                    within(tag + " dw", out["dw"], ref_dw, rel_err(y_dw, ref_dw)) / 4.0,
                    within(tag + " domega", out["dom"], ref_dom, rel_err(y_dom, ref_dom)) / 4.0)
    print("WORST cond %s n=%d: %.2f of the bound" % (kernel, n, worst))
    at_defaults(L)


# ================================================================ 2.6 the fused launches
FUSED_G = {3: (2.0, -1.0, -1.0), 4: (1.0, 1.0, -1.0, -1.0)}


def fused_solve(L, C, Lit, Lmin):
    """One fused launch (solves, combination and reverse sweep) on 3 or 4 problems, as tests/test_gpu_fused_roles.py:_solve
    calls it, every buffer guarded."""
    nprob, n, _ = C.shape
    bufs = {"C": Buf(C.shape, C), "cost": Buf((nprob,)), "nits": Buf((2 * nprob,), dtype=I32), "loss": Buf((1,)),
            "ticket": Buf((1,), torch.zeros(1, dtype=I32), I32), "dC": Buf(C.shape)}
    P = {k: bf.ptr() for k, bf in bufs.items()}
    assert L.lib.kccot_sinkhorn_fused_eligible(n, Lit) == 1
    if nprob == 3:
        call(L, "kccot_sinkhorn_divergence_fused_f32", P["C"], n, EPS, Lit, Lmin, E.THRESH, P["cost"], P["nits"], P["loss"],
             P["ticket"], P["dC"], None)
    else:
        call(L, "kccot_mixed_sinkhorn_loss_fwd_f32", None, None, n, 0, 0.0, *([None] * 6), 1, 1, EPS, Lit, Lmin, E.THRESH,
             L.MIXED_CMIX_GIVEN, P["C"], None, None, P["dC"], P["cost"], P["nits"], P["loss"], P["ticket"], None, 0, None)
    for k, bf in bufs.items():
        assert bf.guards_intact(), "guard zone of %s overwritten (n=%d)" % (k, n)
    assert int(bufs["ticket"].t) == 0
    flat = bufs["nits"].t.tolist()
    return {"cost": bufs["cost"].t.clone(), "loss": bufs["loss"].t.clone(), "dC": bufs["dC"].t.clone(), "nits": flat[:nprob],
            "executed": flat[nprob:]}


@pytest.mark.parametrize("shortcut", [1, 0])
@pytest.mark.parametrize("roles", [1, 0])
@pytest.mark.parametrize("nprob", [3, 4])
@pytest.mark.parametrize("n", E.FUSED_SIZES)
def test_fused_launches_stop_early(L, n, nprob, roles, shortcut):
    """sinkhorn_fused_roles (roles = 1) and sinkhorn_fused_reg (0): counts, costs, loss and dC_unit against float64; against the
    launch with L = Lmin = k[p] bit for bit; and against the two-kernel path (kccot_sinkhorn_fwd_f32 / _bwd_f32 with the
    combination's weights as gcost) bit for bit at sinkhorn_lanes_per_line = 8."""
    at_defaults(L)
    C = E.fused_problems(n)[:nprob].contiguous()
    g = FUSED_G[nprob]
    r64 = E.fused_references(n, g)
    ks = [r[1] for r in r64]
    tag = "fused n=%d nprob=%d roles=%d shortcut=%d" % (n, nprob, roles, shortcut)
    with L.options(sinkhorn_fused_roles=roles, sinkhorn_shortcut=shortcut, sinkhorn_lanes_per_line=8):
        assert L.lib.kccot_sinkhorn_fused_roles_eligible(n, LIT) == roles
        out = fused_solve(L, C, LIT, LMIN)
        print("%s: float64 counts %s, device %s, executed %s" % (tag, ks, out["nits"], out["executed"]))
        assert out["nits"] == ks and len(set(ks)) >= 2, (tag, out["nits"], ks)                                   # 1
        assert out["executed"] == ks if not shortcut else all(0 < e <= k for e, k in zip(out["executed"], ks)), out["executed"]
        for p, k in enumerate(ks):                                                                # 2
            one = fused_solve(L, C, k, k)
            assert one["nits"] == [k] * nprob
            assert same_bits(one["cost"][p], out["cost"][p]) and same_bits(one["dC"][p], out["dC"][p]), (tag, p, k)
        two = solve(L, C, None, None, EPS, LIT, LMIN, E.THRESH, gcost=g)
        assert two["nits"] == ks
        assert same_bits(two["cost"], out["cost"]), tag + ": costs differ from the two-kernel path"
        assert same_bits(two["dC"], out["dC"]), tag + ": dC_unit differs from the two-kernel path"
    at_defaults(L)
    worst = 0.0
    for p, k in enumerate(ks):                                                                     # 3
        cost_err = abs(float(out["cost"][p]) - float(r64[p][0])) / abs(float(r64[p][0]))
        dC_err = rel_err(out["dC"][p], r64[p][2])
        print("%s p=%d k=%d: cost err %.3e (bound %g)  dC_unit err %.3e (bound %g)" % (tag, p, k, cost_err, COST_RTOL, dC_err, DC_ATOL))
        assert cost_err <= COST_RTOL and dC_err <= DC_ATOL and bool(torch.isfinite(out["dC"][p]).all())
        worst = max(worst, cost_err / COST_RTOL, dC_err / DC_ATOL)
    ref_loss = sum(x * r[0] for x, r in zip(g, r64))               # the combination's weights are its upstream gradients
    loss_err = abs(float(out["loss"]) - float(ref_loss)) / abs(float(ref_loss))
    print("%s loss err %.3e (bound %g)" % (tag, loss_err, LOSS_RTOL))
    assert loss_err < LOSS_RTOL
    worst = max(worst, loss_err / LOSS_RTOL)
    print("WORST %s: %.2f of the bound" % (tag, worst))


# ================================================================ 2.7 the boundaries on the device
BOUNDARY = [(48, "uniform", {}, "reg"), (260, "uniform", {"sinkhorn_coop": 0}, "stream gen16<8>"), (260, "uniform", {}, "coop ll<8>"),
            (48, "ab", {}, "reg_w")]


@pytest.mark.parametrize("n,kind,opts,family", BOUNDARY)
def test_boundaries_of_the_stop_rule_on_the_device(L, n, kind, opts, family):
    """Per problem, alone: L = k and L = k + 1 both give k; Lmin = k + 2 gives k + 2 under STOP_COUNT and k + 3 under
    STOP_INDEX; STOP_INDEX at Lmin = 3 gives k.  Each against stopped_sweep with the same arguments, gradients included."""
    at_defaults(L)
    ks = E.references(n, kind, GCOST)[1]
    thresh = E.stop_thresh(n, kind)
    jump = n <= 128
    for p in range(3):
        k = ks[p]
        C, a, b = launch_inputs(n, kind, (p,))
        for Lit, Lmin, mode, want in ((k, LMIN, STOP_COUNT, k), (k + 1, LMIN, STOP_COUNT, k), (LIT, k + 2, STOP_COUNT, k + 2),
                                      (LIT, k + 2, STOP_INDEX, k + 3), (LIT, LMIN, STOP_INDEX, k)):
            tag = "%s p=%d L=%d Lmin=%d mode=%d" % (family, p, Lit, Lmin, mode)
            r64 = E.stopped_sweep(C[0], E.uniform(n) if a is None else a[0], E.uniform(n) if b is None else b[0], EPS, Lit, Lmin,
                                  thresh, mode == STOP_INDEX, GCOST[p])
            r32 = E.stopped_sweep(C[0], E.uniform(n) if a is None else a[0], E.uniform(n) if b is None else b[0], EPS, Lit, Lmin,
                                  thresh, mode == STOP_INDEX, GCOST[p], F32)
            assert r64[1] == r32[1] == want, (tag, r64[1], r32[1], want)
            with L.options(**opts):
                out = solve(L, C, a, b, EPS, Lit, Lmin, thresh, mode, (GCOST[p],))
            assert out["nits"] == [want], (tag, out["nits"], want)
            assert out["executed"] == [want] if not jump else 0 < out["executed"][0] <= want, (tag, out["executed"])
            against_fp64("%s n=%d" % (tag, n), out, [r64], [r32], [want])
    at_defaults(L)


# ================================================================ 2.8 through autograd
@pytest.mark.parametrize("n,kind", [(48, "uniform"), (260, "uniform"), (516, "uniform"), (48, "ab"), (260, "ab")])
def test_wrappers_hand_the_count_to_the_backward(L, n, kind):
    """_Sinkhorn / _WeightedSinkhorn size the history for L = 40 and pass the forward's counts to the reverse sweep."""
    from kccotgan_amd import gan_utils as G
    at_defaults(L)
    assert E.stop_thresh(n, kind) == E.THRESH
    idx = (0, 1, 2) if n < 512 else two_with_different_counts(n, kind)
    C, a, b = launch_inputs(n, kind, idx)
    r64 = list(zip(*E.references(n, kind, GCOST)))
    r32 = list(zip(*E.references(n, kind, GCOST, dtype=F32)))
    ks = [r64[p][1] for p in idx]
    Cd = C.to(DEV).requires_grad_(True)
    up = torch.tensor([GCOST[p] for p in idx], device=DEV)
    tag = "early_stop_%d_%s" % (n, kind)
    if kind == "uniform":
        cost = G._Sinkhorn.apply(Cd, EPS, LIT, LMIN, STOP_COUNT, tag)
    else:
        ad, bd = a.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
        cost = G._WeightedSinkhorn.apply(Cd, ad, bd, EPS, LIT, LMIN, STOP_COUNT, tag)
    (cost * up).sum().backward()
    torch.cuda.synchronize()
    print("%s: float64 counts %s, device %s" % (tag, ks, G.last_info[tag].tolist()))
    assert G.last_info[tag].tolist() == ks and all(0 < e <= k for e, k in zip(G.last_info[tag + "_executed"].tolist(), ks))
    for pos, p in enumerate(idx):
        cost_err = abs(float(cost[pos].detach()) - float(r64[p][0])) / abs(float(r64[p][0]))
        dC_err = rel_err(Cd.grad[pos], r64[p][2])
        print("%s p=%d: cost err %.3e (bound %g)  C.grad err %.3e (bound %g)" % (tag, p, cost_err, COST_RTOL, dC_err, DC_ATOL))
        assert cost_err <= COST_RTOL and dC_err <= DC_ATOL
        if kind != "uniform":
            within("%s p=%d a.grad" % (tag, p), ad.grad[pos], r64[p][3], rel_err(r32[p][3], r64[p][3]))
            within("%s p=%d b.grad" % (tag, p), bd.grad[pos], r64[p][4], rel_err(r32[p][4], r64[p][4]))
    at_defaults(L)


def test_public_loss_stops_at_lmin_when_allowed_more(L):
    """compute_sinkhorn_loss(..., honor_eps_l=True) at B = 132, eps = 1, L = 130: the three solves (multi-CU solver) stop after
    Lmin = 100 iterations, where the float64 oracle's loss ends, in a history sized for 130; loss and gradients against float64
    autograd with the bounds of test_fused_path_at_degenerate_and_late_stopping_iteration_counts."""
    from kccotgan_amd import gan_utils as G
    from oracle import gan_utils_torch as ot
    from test_gpu_fullsize_grads import GRAD_TOL_FLOOR
    at_defaults(L)
    wrt = ("fake", "h_fake", "m_real")
    inp = E.api_inputs()
    t = {k: v.to(DEV).requires_grad_(k in wrt) for k, v in inp.items()}
    loss = G.compute_sinkhorn_loss(t["real"], t["fake"], E.W.cases.SC, E.API_EPS, E.API_L, t["h_fake"], t["m_real"], t["h_real"],
                                   t["m_fake"], honor_eps_l=True)
    grads = torch.autograd.grad(loss, [t[k] for k in wrt])
    torch.cuda.synchronize()
    counts = G.last_info["compute_sinkhorn_loss"].reshape(-1).tolist()[:3]
    print("compute_sinkhorn_loss B=132 L=130: counts %s executed %s" % (counts, G.last_info["compute_sinkhorn_loss_executed"].tolist()))
    assert counts == [100, 100, 100]
    d = {k: v.double().requires_grad_(k in wrt) for k, v in inp.items()}
    ref = ot.compute_sinkhorn_loss(d["real"], d["fake"], E.W.cases.SC, E.API_EPS, E.API_L, d["h_fake"], d["m_real"], d["h_real"],
                                   d["m_fake"])
    gref = torch.autograd.grad(ref, [d[k] for k in wrt])
    err = abs(float(loss) - float(ref)) / abs(float(ref))
    print("loss %.6f float64 %.6f rel %.3e (bound 1e-4)" % (float(loss), float(ref), err))
    assert err < 1e-4
    for k, got, want in zip(wrt, grads, gref):
        e = rel_err(got, want)
        print("d%s err %.3e (bound %g)" % (k, e, 4 * GRAD_TOL_FLOOR))
        assert e <= 4 * GRAD_TOL_FLOOR, (k, e)
    at_defaults(L)
