"""Every kernel instantiation a WEIGHTED Sinkhorn solve can be dispatched to, held to float64 (the sizes of
tests/test_gpu_weighted_sinkhorn.py, (5, 64, 67, 128, 130), reach only a few of them).

Size and options -> kernel, read from the dispatch code (file:line of the rule):

  streaming forward, n > 128 (kccotgan_amd/csrc/sinkhorn_gen.hip:627-632; weighted work never takes the multi-CU solver, :618)
    n            C 16-byte aligned   forward kernel               tested in modes (w_div)
    131, 1023    yes                 sinkhorn_fwd_gen<true>       0 (1, 2: n = 130 in   n % 4 != 0                       (:629)
                                                                  the older files)
    132          no (4 bytes off)    sinkhorn_fwd_gen<true>       0                     (uintptr_t)C % 16 != 0           (:627)
    132, 256     yes                 sinkhorn_fwd_gen16<4,true>   0; 132 also 1 and 2   n % 4 == 0, n <= 256             (:630)
    260, 512     yes                 sinkhorn_fwd_gen16<8,true>   0; 260 also 1 and 2   n % 4 == 0, n <= 512             (:631)
    516, 1024    yes                 sinkhorn_fwd_gen4<4,true>    0; 516 also 1 and 2   n % 4 == 0, n <= 1024 = SG_MAXN  (:632)
  streaming backward, every n > 128: sinkhorn_bwd_gen<true> (_bwd_f32, :659) and sinkhorn_bwd_gen<true,true> (_bwd_dw_f32, :658);
    n = 1024 fills every SG_MAXN array of LDS exactly, n = 1025 is refused (:614, :645)
  the unweighted twins that give the yardstick at n > 128 run under sinkhorn_coop = 0 (:635-638)

  register path, n <= 128 (kccotgan_amd/csrc/sinkhorn.hip: lanes per line :1263, option sinkhorn_lanes_per_line at
  32 < n <= 64 :1264-1269, entries per lane :1270-1271, <EPT,LPR> switch :1302-1316; sinkhorn_shortcut = 1 -> sinkhorn_fwd_reg_w,
  0 -> sinkhorn_fwd_reg_full_w :1346-1351; backward sinkhorn_bwd_reg_dw :1406-1408, sinkhorn_bwd_reg_w :1410-1412)
    n            sinkhorn_lanes_per_line   forward <EPT,LPR>   backward <EPT,LPR>
    7            0                         <1,16>              <1,16>        (section 3 only)
    17, 24, 32   0                         <2,16>              <2,16>
    33           0                         <8,8>               <4,16>        (section 3 only)
    48           0                         <8,8>               <4,16>
    48           4                         <16,4>              <16,4>
    48           8                         <8,8>               <8,8>
    48           16                        <4,16>              <4,16>
    64           0                         <8,8>               <4,16>
    100, 128     0                         <16,8>              <16,8>
  Sections 2 and 3 run each row with sinkhorn_shortcut = 1 (_w) and = 0 (_full_w): all six shapes in the forward, in
  sinkhorn_bwd_reg_w and in sinkhorn_bwd_reg_dw, and sinkhorn_fwd_reg_full_w in all six.
  the shortcut's jump (sinkhorn.hip:306-331: the history filled from the ring, the loop resumed at K1) fires in section 3:
  every test there asserts executed < nits.  It also fires in section 2 at (eps, L) = (1.0, 100), with UNEQUAL row and column
  weights: on the device most of the small_cost problems reach a float32 fixed point after 10 to 26 iterations.

Tolerances are those of the three existing files, not new ones.  Costs and dC:
    |got - ref| <= 4 max(yardstick, 2^-24) max|ref|,
the yardstick being the relative error of the UNWEIGHTED entry points (the parent's kernels) on the same matrices against float64;
at n > 128 they run under sinkhorn_coop = 0, so that the figure comes from the unweighted twin of the same kernel family, and the
default (multi-CU) solver's figure is printed beside it.  da, db and the end-to-end weight gradients: the yardstick is the plain
torch sweep of tests/test_weight_grad_cpu.py in float32 against its own float64 run.  Every test prints error, yardstick and
ratio before it asserts (-s); DESIGN.md records the worst ratio per instantiation.

The float64 reference of the solver tests is that same sweep in float64: it keeps no autograd tape (three tapes through 20
iterations at n = 1024 are GBs), and where a tape is cheap (n <= 260, L = 7) it is asserted equal to float64 autograd
(GW.reference, solver_reference) to 1e-9.  L <= Lmin = 100 throughout sections 1 and 2, so the count is L: nits_out[p] == L is
asserted everywhere, nits_out[nprob + p] == L wherever no jump is possible (streaming kernels, sinkhorn_shortcut = 0, L = 7).

Every test reads its options on entry and fails unless they are at their defaults; options are set through L.options(...) only.
Every buffer handed to the C ABI lies between NaN-filled guard zones and workspaces are exactly as long as the queries say.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_conditional_sinkhorn as GC
import test_gpu_weight_grad as GD
import test_gpu_weighted_sinkhorn as GW
import test_weighted_sinkhorn_cpu as W
from test_gpu_conditional_sinkhorn import problem
from test_gpu_weight_grad import solve_dw, solver_reference, solver_yardstick
from test_gpu_weighted_sinkhorn import (Buf, solve, call, within, rel_err, same_bits, problems, reference, workspace, GCOST,
                                        loss_inputs, run_loss, loss_reference_with)
from test_weight_grad_cpu import sweep
from test_weighted_sinkhorn_cpu import weighted_sinkhorn, random_weights, small_cost, F64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
I32 = torch.int32
DEFAULTS = {"sinkhorn_shortcut": 1, "sinkhorn_coop": 1, "sinkhorn_lanes_per_line": 0, "sinkhorn_fused": 1}
STOP_COUNT, STOP_INDEX = 0, 1


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    assert (_lib.STOP_COUNT, _lib.STOP_INDEX) == (STOP_COUNT, STOP_INDEX)
    return _lib


def at_defaults(L):
    got = {k: L.get_option(k) for k in DEFAULTS}
    assert got == DEFAULTS, "options not at their defaults on entry: %s" % got


# ---------------------------------------------------------------- float64 references (the sweep), computed once
@functools.lru_cache(maxsize=None)
def sweeps(n, eps, Lit, uniform):
    """float64 (cost [3], dC [3,n,n], da [3,n], db [3,n]) of sum_p GCOST[p] W(C_p; a_p, b_p) on the float32 inputs of problems(n),
    by the tape-free sweep; uniform: a = b = 1/n (the reference of the yardstick's unweighted run)."""
    C, a, b = problems(n)
    uni = torch.full((n,), 1.0 / n, dtype=F64)
    r = [sweep(C[p], uni if uniform else a[p], uni if uniform else b[p], eps, Lit, g=GCOST[p]) for p in range(3)]
    assert [x[1] for x in r] == [Lit] * 3
    out = tuple(torch.stack([x[k] for x in r]) for k in (0, 2, 3, 4))
    if n <= 260 and Lit == 7:          # a tape is cheap here: the sweep IS float64 autograd
        auto = reference(n, eps, Lit, uniform)
        assert auto[1] == [Lit] * 3 and rel_err(out[0], auto[0]) <= 1e-9 and rel_err(out[1], auto[2]) <= 1e-9
        if not uniform:
            ra, rb = solver_reference(n, eps, Lit)
            assert rel_err(out[2], ra) <= 1e-9 and rel_err(out[3], rb) <= 1e-9
    return out


def test_inputs_meet_the_conditions_of_the_tolerances(L):
    """Every float32 weight the device reads is positive and normal, and the weighted loop in float64 runs its L iterations."""
    at_defaults(L)
    for n in (17, 24, 32, 48, 64, 128, 131, 132, 256, 260, 512, 516, 1023, 1024):
        _, a, b = problems(n)
        tiny = float(torch.finfo(F32).tiny)
        assert float(a.min()) >= tiny and float(b.min()) >= tiny, n
    for n in (132, 260, 516):
        _, w, _ = problem(n)
        assert float(w.min()) >= float(torch.finfo(F32).tiny)
    C, a, b = problems(24)
    assert weighted_sinkhorn(C[0].double(), a[0].double(), b[0].double(), 1.0, 100)[1] == 100
    assert tuple(small_cost(24, 2400).shape) == (24, 24) and abs(float(random_weights(24, 1).sum()) - 1.0) < 1e-12


_YARD = {}


def unweighted_yardstick(L, n, eps, Lit, c_off=0):
    """Relative error (cost, dC) of kccot_sinkhorn_fwd_f32 / _bwd_f32 on the matrices of problems(n) against float64; at n > 128
    under sinkhorn_coop = 0 (the unweighted twin of the streaming kernel), the default solver's figures printed beside."""
    key = (n, eps, Lit, c_off)
    if key not in _YARD:
        C, _, _ = problems(n)
        ref = sweeps(n, eps, Lit, True)
        with L.options(sinkhorn_coop=0):
            cost, nits, dC = solve(L, C, None, None, eps, Lit, c_off=c_off)
        assert nits[:3].tolist() == [Lit] * 3
        _YARD[key] = (rel_err(cost, ref[0]), rel_err(dC, ref[1]))
        if n > 128:
            cost, nits, dC = solve(L, C, None, None, eps, Lit, c_off=c_off)
            assert nits[:3].tolist() == [Lit] * 3
            print("n=%d eps=%g L=%d unweighted: one-workgroup solver cost %.3e dC %.3e | default solver cost %.3e dC %.3e"
                  % ((n, eps, Lit) + _YARD[key] + (rel_err(cost, ref[0]), rel_err(dC, ref[1]))))
    return _YARD[key]


def check_solver(L, tag, n, eps, Lit, c_off=0, **opts):
    """The three weighted solver entry points on problems(n), run under the options `opts`, against float64: cost, nits, dC, da,
    db.  Every iteration executes, unless the periodic-state shortcut is on and L = 100: at eps = 1 the register kernels reach a
    float32 fixed point on most of these matrices after 10 to 26 iterations and jump (measured: executed = 15, 10, 12 at n = 17;
    14, 100, 100 at n = 24 and 48; 16, 15, 24 at n = 128), which the comparison against sinkhorn_shortcut = 0 then covers as well.
    The yardsticks are taken at the default options.  Returns every output."""
    C, a, b = problems(n)
    ref = sweeps(n, eps, Lit, False)
    yard_c, yard_d = unweighted_yardstick(L, n, eps, Lit, c_off)
    yard_a, yard_b = solver_yardstick(n, eps, Lit)
    with L.options(**opts):
        out = solve_dw(L, C, a, b, eps, Lit, c_off=c_off)
    nits, executed = out["nits"][:3].tolist(), out["nits"][3:].tolist()
    print("%s n=%d eps=%g L=%d nits %s executed %s" % (tag, n, eps, Lit, nits, executed))
    assert nits == [Lit] * 3, (tag, nits)
    if n > 128 or Lit < 100 or opts.get("sinkhorn_shortcut", 1) == 0:
        assert executed == [Lit] * 3, (tag, executed)
    else:
        assert all(0 < e <= Lit for e in executed), (tag, executed)
    assert same_bits(out["dC"], out["dC0"]), tag + ": dC of the _dw call differs from kccot_sinkhorn_weighted_bwd_f32"
    head = "%s n=%d eps=%g L=%d " % (tag, n, eps, Lit)
    r = [within(head + k, out[k], x, y) for k, x, y in (("cost", ref[0], yard_c), ("dC", ref[1], yard_d), ("da", ref[2], yard_a),
                                                         ("db", ref[3], yard_b))]
    print("WORST %s n=%d: cost/dC %.2f  da/db %.2f" % (tag, n, max(r[:2]), max(r[2:])))
    return out


def settings(n):
    return [(0.8, 7)] + ([(1.0, 100)] if n <= 260 else []) + ([(0.8, 20)] if n >= 512 else [])


# ================================================================ 1. the streaming solver: every forward kernel
STREAM = [(131, 0, "gen"), (132, 0, "gen16<4>"), (132, 1, "gen(C+4B)"), (256, 0, "gen16<4>"), (260, 0, "gen16<8>"), (512, 0, "gen16<8>"),
          (516, 0, "gen4<4>"), (1023, 0, "gen"), (1024, 0, "gen4<4>")]


@pytest.mark.parametrize("n,c_off,kernel,eps,Lit", [c + s for c in STREAM for s in settings(c[0])])
def test_streaming_solver_against_fp64(L, n, c_off, kernel, eps, Lit):
    at_defaults(L)
    out = check_solver(L, kernel, n, eps, Lit, c_off)
    if c_off:       # the narrow kernel reads the same numbers in another order: close to the wide kernel's answer, not its bits
        wide = solve_dw(L, *problems(n), eps, Lit)
        assert rel_err(out["cost"], wide["cost"].double().cpu()) <= 1e-5 and not same_bits(out["u"], wide["u"])


COND_Q, COND_EPS, COND_L = 2, 0.8, 10


@functools.lru_cache(maxsize=None)
def cond_pieces(n, dtype):
    """Per (q, k): cost, dcost/dC3[k] and da + db of W(C3[k]; w_q, w_q) at g = 1 by the torch sweep in `dtype`."""
    C3, w, _ = problem(n)
    cost = torch.zeros(COND_Q, 3, dtype=dtype)
    dC = torch.zeros(COND_Q, 3, n, n, dtype=dtype)
    dw = torch.zeros(COND_Q, 3, n, dtype=dtype)
    for q in range(COND_Q):
        for k in range(3):
            r = sweep(C3[k], w[q], w[q], COND_EPS, COND_L, dtype=dtype)
            assert r[1] == COND_L
            cost[q, k], dC[q, k], dw[q, k] = r[0], r[2], r[3] + r[4]
    return cost, dC, dw


@pytest.mark.parametrize("n,kernel", [(132, "gen16<4>"), (260, "gen16<8>"), (516, "gen4<4>")])
def test_streaming_conditional_solver_against_fp64(L, n, kernel):
    """w_div = 2: Q = 2 weight rows on the shared C3 (the matrices of problems(n))."""
    at_defaults(L)
    C3, w, omega = problem(n)
    assert same_bits(C3, problems(n)[0])
    w = w[:COND_Q].contiguous()
    p64, p32 = cond_pieces(n, F64), cond_pieces(n, F32)
    yard_c, yard_d = unweighted_yardstick(L, n, COND_EPS, COND_L)
    worst = 0.0
    for om, gl in ((None, 1.0), ((omega[:COND_Q] / omega[:COND_Q].sum()).contiguous(), -0.5)):
        tag = "%s w_div=2 n=%d omega=%s gloss=%g " % (kernel, n, "1/Q" if om is None else "given", gl)
        out = GD.cond_solve_dw(L, C3, w, om, COND_EPS, COND_L, gl)
        assert out["nits"].tolist() == [[[COND_L] * 3] * COND_Q] * 2
        assert same_bits(out["dC3"], out["dC0"]), tag + ": dC3 differs from kccot_sinkhorn_conditional_bwd_f32"
        _, ref_dC = GC.combine64(p64[0], p64[1], om, COND_Q, gl)
        ref_dw, ref_dom = GD.cond_combine((p64[0], p64[2]), om, COND_Q, gl)
        y_dw, y_dom = GD.cond_combine((p32[0], p32[2]), om, COND_Q, gl)
        assert bool(torch.isfinite(out["loss"]).all())
        worst = max(worst, within(tag + "costs", out["cost"], p64[0], yard_c), within(tag + "dC3", out["dC3"], ref_dC, yard_d))
        r = max(within(tag + "dw (da+db)", out["dw"], ref_dw, rel_err(y_dw, ref_dw)),
                within(tag + "domega", out["dom"], ref_dom, rel_err(y_dom, ref_dom)))
        print("WORST %s w_div=2 n=%d: cost/dC %.2f  dw %.2f" % (kernel, n, worst, r))


@pytest.mark.parametrize("B,kernel", [(132, "gen16<4>"), (260, "gen16<8>"), (516, "gen4<4>")])
def test_streaming_weighted_loss_against_fp64(L, B, kernel):
    """w_div = 1: compute_weighted_sinkhorn_loss, with and without a gradient w.r.t. the weights."""
    from kccotgan_amd import gan_utils as g
    at_defaults(L)
    shape, Lit = (B, 2, 4, 4, 1, 2), 10
    t = loss_inputs(shape)
    uni = torch.full((B,), 1.0 / B, dtype=F64)
    ref_u = loss_reference_with(shape, uni, uni, Lit)
    ref_w = loss_reference_with(shape, t["w_real"].double(), t["w_fake"].double(), Lit)
    ref_dw, yard_dw = GD.loss_weight_reference(shape, False, 1.0, Lit)
    with L.options(sinkhorn_coop=0):
        got_u = run_loss(shape, Lit=Lit)
    got_d = run_loss(shape, Lit=Lit)
    yard = [rel_err(x, r.reshape(x.shape)) for x, r in zip(got_u, ref_u)]
    print("B=%d unweighted loss: one-workgroup solver %s | default solver %s"
          % (B, " ".join("%.2e" % y for y in yard), " ".join("%.2e" % rel_err(x, r.reshape(x.shape)) for x, r in zip(got_d, ref_u))))
    plain = run_loss(shape, t["w_real"], t["w_fake"], Lit=Lit)
    tag = "compute_weighted_sinkhorn_loss"
    assert g.last_info[tag + "_path"] == "streaming" and g.last_info[tag].tolist() == [Lit] * 3
    withw = run_loss(shape, t["w_real"], t["w_fake"], Lit=Lit, weight_grads=True)
    assert g.last_info[tag + "_path"] == "streaming" and g.last_info[tag].tolist() == [Lit] * 3
    assert g.last_info[tag + "_executed"].tolist() == [Lit] * 3
    for k, x, y in zip(GW.NAMES, plain, withw):
        assert same_bits(x.reshape(-1), y.reshape(-1)), "%s changes when the weights require a gradient" % k
    head = "%s w_div=1 B=%d " % (kernel, B)
    r1 = max(within(head + k, x, r.reshape(x.shape), y) for k, x, r, y in zip(GW.NAMES, withw, ref_w, yard))
    r2 = max(within(head + "dw_real", withw[6], ref_dw[0], yard_dw[0]), within(head + "dw_fake", withw[7], ref_dw[1], yard_dw[1]))
    print("WORST %s w_div=1 B=%d: loss and gradients %.2f  dw %.2f" % (kernel, B, r1, r2))


# ================================================================ 2. the register path: the shapes the size list misses
REG = [(17, 0, "<2,16>/<2,16>"), (24, 0, "<2,16>/<2,16>"), (32, 0, "<2,16>/<2,16>"), (48, 0, "<8,8>/<4,16>"), (48, 4, "<16,4>/<16,4>"),
       (48, 8, "<8,8>/<8,8>"), (48, 16, "<4,16>/<4,16>"), (64, 0, "<8,8>/<4,16>"), (128, 0, "<16,8>/<16,8>")]
OUTS = ("cost", "u", "v", "dC0", "dC", "da", "db")


@pytest.mark.parametrize("eps,Lit", [(0.8, 7), (1.0, 100)])
@pytest.mark.parametrize("n,lanes,shapes", REG)
def test_register_shapes_against_fp64_with_and_without_the_shortcut(L, n, lanes, shapes, eps, Lit):
    """sinkhorn_shortcut = 1 runs sinkhorn_fwd_reg_w, 0 sinkhorn_fwd_reg_full_w, and the two agree in every output bit.  At L = 7
    both execute every iteration; at L = 100 the run without the shortcut does, the other may jump (see check_solver)."""
    at_defaults(L)
    runs = {}
    for sc in (1, 0):
        runs[sc] = check_solver(L, "%s lanes=%d shortcut=%d" % (shapes, lanes, sc), n, eps, Lit, sinkhorn_lanes_per_line=lanes,
                                sinkhorn_shortcut=sc)
    at_defaults(L)
    for k in OUTS:
        assert same_bits(runs[1][k], runs[0][k]), "%s differs between sinkhorn_shortcut = 1 and 0" % k
    assert runs[1]["nits"][:3].tolist() == runs[0]["nits"][:3].tolist() == runs[0]["nits"][3:].tolist() == [Lit] * 3
    assert bool(torch.isfinite(runs[1]["u"]).all()) and bool(torch.isfinite(runs[1]["v"]).all())


def test_lanes_per_line_changes_the_kernel_not_the_answer(L):
    """n = 48 under 4, 8 and 16 lanes per line: three different summation trees (other bits somewhere), one answer."""
    at_defaults(L)
    C, a, b = problems(48)
    outs = []
    for lanes in (4, 8, 16):
        with L.options(sinkhorn_lanes_per_line=lanes):
            outs.append(solve_dw(L, C, a, b, 1.0, 100))
    assert not all(same_bits(outs[0][k], o[k]) for o in outs[1:] for k in ("u", "dC", "da"))
    for o in outs[1:]:
        for k in ("cost", "dC", "da", "db"):
            assert rel_err(o[k], outs[0][k].double().cpu()) <= 1e-4, k


# ================================================================ 3. the shortcut's jump with weights is exact
JUMP = ((7, 300.0), (24, 500.0), (33, 500.0), (64, 2000.0), (100, 3000.0))
JUMP_SETTINGS = ((1.0, 100, 100, STOP_COUNT), (1.0, 7, 100, STOP_COUNT), (0.8, 50, 20, STOP_INDEX), (0.5, 40, 3, STOP_COUNT))


@functools.lru_cache(maxsize=None)
def jump_problem(n, scale):
    """Three symmetric matrices C = scale |x_i - x_j|^2 (zero diagonal, smallest off-diagonal entry >= 30 eps) and three weight
    vectors used for BOTH marginals: the xx / yy problems of the weighted divergence and of the conditional loss."""
    Cs, ws = [], []
    for p in range(3):
        x = np.random.default_rng(1000 * n + p).random((n, 6))
        C = (scale * ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)).astype(np.float32)
        assert np.array_equal(C, C.T) and not C.diagonal().any()
        assert float(C[~np.eye(n, dtype=bool)].min()) >= 30.0 * max(s[0] for s in JUMP_SETTINGS)
        Cs.append(torch.from_numpy(C))
        ws.append(random_weights(n, 500 + 10 * n + p).float())
    return torch.stack(Cs), torch.stack(ws)


def split_nits(nits, nprob):
    flat = nits.reshape(-1).tolist()
    return flat[:nprob], flat[nprob:]


@pytest.mark.parametrize("n,scale", JUMP)
def test_weighted_jump_is_bit_exact(L, n, scale):
    """Weighted solver entry points, sinkhorn_shortcut = 1 against 0: cost, nits, the whole histories (rows past nits keep their
    NaN prefill in both), dC, da, db.  The run with the shortcut must have skipped iterations."""
    at_defaults(L)
    C, w = jump_problem(n, scale)
    jumped = False
    for eps, Lit, Lmin, mode in JUMP_SETTINGS:
        runs = {}
        for sc in (1, 0):
            with L.options(sinkhorn_shortcut=sc):
                runs[sc] = solve_dw(L, C, w, w, eps, Lit, Lmin=Lmin, stop_mode=mode)
        tag = (n, eps, Lit, Lmin, mode)
        (nits1, exe1), (nits0, exe0) = split_nits(runs[1]["nits"], 3), split_nits(runs[0]["nits"], 3)
        print("n=%d eps=%g L=%d Lmin=%d mode=%d: nits %s executed with the shortcut %s" % (tag + (nits1, exe1)))
        assert nits1 == nits0 and exe0 == nits0 and all(0 < e <= k for e, k in zip(exe1, nits1)), tag
        jumped |= any(e < k for e, k in zip(exe1, nits1))
        for k in ("cost", "u", "v", "dC0", "dC", "da", "db"):
            assert same_bits(runs[1][k], runs[0][k]), (tag, k)
        for p in range(3):
            assert bool(torch.isfinite(runs[1]["u"][p, :nits1[p]]).all()) and bool(torch.isfinite(runs[1]["da"]).all()), tag
            assert bool(torch.isnan(runs[1]["u"][p, nits1[p]:]).all()) and bool(torch.isnan(runs[1]["v"][p, nits1[p]:]).all()), tag
    assert jumped, "no problem at n=%d skipped an iteration: the jump was not exercised" % n
    at_defaults(L)


@pytest.mark.parametrize("n,scale", JUMP)
def test_conditional_jump_is_bit_exact(L, n, scale):
    """The same through the conditional solver: Q = 2 weight rows, each both marginals of its three problems (count-based stop
    rule only: the INDEX setting runs with its eps, L and Lmin)."""
    at_defaults(L)
    C3, w = jump_problem(n, scale)
    w = w[:2].contiguous()
    jumped = False
    for eps, Lit, Lmin, _ in JUMP_SETTINGS:
        runs = {}
        for sc in (1, 0):
            with L.options(sinkhorn_shortcut=sc):
                runs[sc] = GD.cond_solve_dw(L, C3, w, None, eps, Lit, 1.0, Lmin=Lmin)
        tag = (n, eps, Lit, Lmin)
        (nits1, exe1), (nits0, exe0) = split_nits(runs[1]["nits"], 6), split_nits(runs[0]["nits"], 6)
        print("n=%d eps=%g L=%d Lmin=%d: nits %s executed with the shortcut %s" % (tag + (nits1, exe1)))
        assert nits1 == nits0 and exe0 == nits0 and all(0 < e <= k for e, k in zip(exe1, nits1)), tag
        jumped |= any(e < k for e, k in zip(exe1, nits1))
        for k in ("cost", "loss", "u", "v", "dC0", "dC3", "dw", "dom"):
            assert same_bits(runs[1][k], runs[0][k]), (tag, k)
        assert bool(torch.isfinite(runs[1]["dw"]).all()) and bool(torch.isfinite(runs[1]["dC3"]).all()), tag
    assert jumped, "no problem at n=%d skipped an iteration: the jump was not exercised" % n
    at_defaults(L)


def test_weighted_loss_is_bit_identical_with_and_without_the_jump(L):
    """compute_weighted_sinkhorn_loss on sharp inputs (deci64 videos, costs of O(1e2..1e3) against eps = 1), the weights
    requiring a gradient: loss, dfake, the four feature gradients, dw_real and dw_fake."""
    from kccotgan_amd import gan_utils as g
    at_defaults(L)
    inp = {k: torch.from_numpy(v) for k, v in W.cases.gen_inputs("deci64", 1, "far").items()}
    B = inp["real"].shape[0]
    assert B == 64
    wr0, wf0 = random_weights(B, 71).float(), random_weights(B, 72).float()
    tag = "compute_weighted_sinkhorn_loss"
    runs, info = {}, {}
    for sc in (1, 0):
        with L.options(sinkhorn_shortcut=sc):
            real = inp["real"].to(DEV)
            leaves = [inp[k].to(DEV).requires_grad_(True) for k in ("fake",) + GW.FEATS] + [wr0.to(DEV).requires_grad_(True),
                                                                                           wf0.to(DEV).requires_grad_(True)]
            fake, hf, mr, hr, mf, wr, wf = leaves
            loss = g.compute_weighted_sinkhorn_loss(real, fake, 1.0, 1.0, 100, hf, mr, hr, mf, wr, wf, normalize=False)
            runs[sc] = (loss.detach(),) + torch.autograd.grad(loss, leaves)
            torch.cuda.synchronize()
            info[sc] = (g.last_info[tag].tolist(), g.last_info[tag + "_executed"].tolist(), g.last_info[tag + "_path"])
            C3 = g.last_info[tag + "_C3"]
            print("shortcut=%d: nits %s executed %s, cost entries up to %.0f" % (sc, info[sc][0], info[sc][1], float(C3.max())))
    at_defaults(L)
    assert info[1][2] == info[0][2] == "register"
    assert info[1][0] == info[0][0] == info[0][1] and all(k > 0 for k in info[0][0])
    assert any(e < k for e, k in zip(info[1][1], info[1][0])), "the jump did not fire at the loss level"
    for k, x, y in zip(GW.NAMES + ("dw_real", "dw_fake"), runs[1], runs[0]):
        assert bool(torch.isfinite(x).all()), k
        assert same_bits(x.reshape(-1), y.reshape(-1)), "%s differs between sinkhorn_shortcut = 1 and 0" % k


# ================================================================ 4. edges of the streaming backward
def test_one_past_the_largest_size_is_refused_by_every_entry_point(L):
    at_defaults(L)
    n, nprob, Q, Lit = 1025, 3, 1, 2
    EUNSUPPORTED = L.EUNSUPPORTED
    g = torch.Generator().manual_seed(0)
    Cb = Buf((3, n, n), torch.rand(3, n, n, generator=g))
    ab, bb = (Buf((nprob, n), torch.full((nprob, n), 1.0 / n)) for _ in range(2))
    gb, g1 = Buf((nprob,), torch.tensor(GCOST)), Buf((1,), torch.ones(1))
    hist = {k: Buf((nprob, Lit, n), torch.zeros(nprob, Lit, n)) for k in ("u", "v")}
    nits_in = Buf((2 * nprob,), torch.full((2 * nprob,), Lit, dtype=I32), I32)
    outs = {k: Buf(s) for k, s in (("u", (nprob, Lit, n)), ("v", (nprob, Lit, n)), ("cost", (nprob,)), ("nits", (2 * nprob,)),
                                   ("loss", (1,)), ("dC", (3, n, n)), ("da", (nprob, n)), ("db", (nprob, n)), ("dw", (Q, n)),
                                   ("dom", (Q,)))}
    ws, wsb = workspace(L.lib.kccot_sinkhorn_workspace_bytes(nprob, 1024))
    call(L, "kccot_sinkhorn_weighted_fwd_f32", Cb.ptr(), ab.ptr(), bb.ptr(), nprob, n, 1.0, Lit, W.LMIN, W.THRESH, STOP_COUNT,
         outs["u"].ptr(), outs["v"].ptr(), outs["cost"].ptr(), outs["nits"].ptr(), None, ws.ptr(), wsb, None, want=EUNSUPPORTED)
    call(L, "kccot_sinkhorn_weighted_bwd_f32", Cb.ptr(), ab.ptr(), bb.ptr(), hist["u"].ptr(), hist["v"].ptr(), nits_in.ptr(), nprob, n,
         1.0, Lit, gb.ptr(), outs["dC"].ptr(), ws.ptr(), wsb, None, want=EUNSUPPORTED)
    call(L, "kccot_sinkhorn_weighted_bwd_dw_f32", Cb.ptr(), ab.ptr(), bb.ptr(), hist["u"].ptr(), hist["v"].ptr(), nits_in.ptr(), nprob,
         n, 1.0, Lit, gb.ptr(), outs["dC"].ptr(), outs["da"].ptr(), outs["db"].ptr(), ws.ptr(), wsb, None, want=EUNSUPPORTED)
    # the conditional solver: Q = 1, its three problems on the shared C3
    call(L, "kccot_sinkhorn_conditional_fwd_f32", Cb.ptr(), ab.ptr(), None, Q, n, 1.0, Lit, W.LMIN, W.THRESH, outs["u"].ptr(),
         outs["v"].ptr(), outs["cost"].ptr(), outs["nits"].ptr(), outs["loss"].ptr(), ws.ptr(), wsb, None, want=EUNSUPPORTED)
    call(L, "kccot_sinkhorn_conditional_bwd_f32", g1.ptr(), Cb.ptr(), ab.ptr(), None, hist["u"].ptr(), hist["v"].ptr(), nits_in.ptr(), Q,
         n, 1.0, Lit, outs["dC"].ptr(), ws.ptr(), wsb, None, want=EUNSUPPORTED)
    cost_in = Buf((Q, 3), torch.ones(Q, 3))
    call(L, "kccot_sinkhorn_conditional_bwd_dw_f32", g1.ptr(), Cb.ptr(), ab.ptr(), None, hist["u"].ptr(), hist["v"].ptr(), nits_in.ptr(),
         Q, n, 1.0, Lit, outs["dC"].ptr(), cost_in.ptr(), outs["dw"].ptr(), outs["dom"].ptr(), ws.ptr(), wsb, None, want=EUNSUPPORTED)
    for k, o in outs.items():
        assert o.untouched(), "%s written by a refused call" % k
    assert ws.untouched()


@pytest.mark.parametrize("bad", [0.0, float("nan")])
@pytest.mark.parametrize("n", [24, 256])
def test_a_bad_weight_poisons_its_problem_only(L, n, bad):
    """An ordinary input check of the kernels (<2,16> register shape; sinkhorn_fwd_gen16<4,true> and both streaming sweeps)."""
    at_defaults(L)
    C, a, b = problems(n)
    good = solve_dw(L, C, a, b, 1.0, 7)
    assert good["nits"].tolist() == [7] * 6
    for side in (0, 1):
        a2, b2 = a.clone(), b.clone()
        (a2, b2)[side][1, n // 3] = bad
        out = solve_dw(L, C, a2, b2, 1.0, 7)
        assert bool(torch.isnan(out["cost"][1])) and int(out["nits"][1]) < 0, (out["cost"], out["nits"])
        for k in ("dC0", "dC", "da", "db"):
            assert bool(torch.isnan(out[k][1]).all()), k
        for p in (0, 2):
            assert int(out["nits"][p]) == 7
            for k in ("cost", "u", "v", "dC0", "dC", "da", "db"):
                assert same_bits(out[k][p], good[k][p]), (k, p)
