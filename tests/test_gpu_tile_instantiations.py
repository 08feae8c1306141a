"""Every instantiation of the planner-driven tile kernels -- dsigma_tile<R, NI> (csrc/smooth_sigma.hip), aniso_tile<RS, NI, JOB>
(csrc/smooth_aniso.hip) -- and every tiling regime of these and of ssim_walk<R, BWD> (csrc/ssim.hip), against float64.

The three older modules (test_gpu_smooth_sigma.py, test_gpu_aniso_smoothing.py, test_gpu_ssim.py) run hand-picked small shapes,
at which the planners always choose the smallest tile: one owned position per thread (NI = 1), and never the radii 5 and 6 (SSIM:
2, 4, 6), an interior tile, or the branch that stops cutting H.  Training runs NI = 2 .. 8 (tests/test_tile_plans_cpu.py has
the count).  The cases here come from tests/tile_plan_cases.py: one per instantiation and per regime, found by
tools/find_tile_plan_cases.py through the host-only plan queries.  Each case FIRST asserts through the query that it still
reaches its instantiation or regime -- a re-tuned planner then fails here instead of silently dropping coverage -- and then runs
the kernel against the float64 oracles of the older modules, with their helpers and their bounds unchanged:
    aniso    k_fwd / k_bwd / k_dsigma, check_forward (4e-6 absolute, max == 1, arg-max sets), check_backward (1e-5 max|ref|),
             check_dsigma (1e-5 Y) of test_gpu_aniso_smoothing.py on the tie-free `video` input;
    dsigma   the entry call of test_gpu_smooth_sigma.py and smooth_sigma_oracle.dsigma_ref, 1e-5 Y, for a random upstream
             gradient and for the aligned one of the older grid (gout = ds/dsigma: |ref| >= 0.01 Y; the anisotropic dsigma too);
    ssim     k_fwd / k_bwd (guard zones) of test_gpu_ssim.py against ssim_oracle.scores / mse / adjoint, TOL_SSIM, TOL_MSE, TOL_DY.
The bounds are absolute or relative to a float64 yardstick (Y, max|ref|), so they do not grow with a case.  One sigma (pair) per
case, at which no tap underflows.  Every test prints its error, its bound and their ratio; the module prints the worst ratio
per family at its end (DESIGN.md sections 4.5.3, 4.5.4 and 14 record them).

The flat input through the SSIM backward.  The older grid checks the adjoint on noise only.  tests/test_ssim_cpu.py
(test_flat_adjoint_in_float32_stays_inside_the_cap_except_at_radius_0) shows a plain float32 evaluation of the oracle's adjoint on
the flat input of the radius cases to stay inside CAP_DY = 1e-4 of max|ref| against float64 at the radii 1..7 (at most 8.0e-5),
so those run here under CAP_DY.  At radius 0 it does not (1.0e-3: with one tap of weight 1 the three variances are differences
of equal numbers, which float32 leaves as rounding noise where the kernel writes exact zeros), so the flat adjoint at radius 0
is left out.

No case exposed a kernel defect: all 169 pass on an MI355X (the worst ratios are in DESIGN.md).

MUTANTS.  Arithmetic only -- no address, no bound -- each built once and run once on an MI355X against the three older modules
(199 tests) and this one (169):
    aniso_tile    the H stencil of owned position 1 reads position 0's F window (winF[n == 1 ? 0 : n]):
                  older modules pass; 45 cases fail here (every job at NI > 1).
    aniso_tile    the spatial taps ws[3] and ws[4] swapped on the host at RS = 5:
                  older modules pass; the five forward and dsigma cases at RS = 5 fail here (the adjoint's taps are the border tables).
    dsigma_tile   the H stencil of owned position 1 reads position 0's G window (winG[n == 1 ? 0 : n]):
                  24 cases fail here -- and two of test_gpu_smooth_sigma.py, whose (1,2,9,40,300) case at r = 1 is the one <1, 2>
                  the older grid reaches.  Restricted to R >= 2: older modules pass; 20 cases fail here.
                  With the random gout alone the unrestricted mutant passed <2, 4> and <3, 4> at (3,16,30,64,16): a quarter of
                  1.5 M random-sign terms against 1e-5 of the sum of their absolute values.  Hence the aligned gout in every case.
    ssim_walk     backward, u gamma dropped in interior tiles (cg = 0 where xcol0 > 0 and q0 + wt < W - 2r):
                  older modules pass (none has three column tiles); ntw3 fails here, |dy - ref| = 0.35 max|ref|."""
import functools

import pytest
import torch

import smooth_aniso_oracle as ao
import smooth_sigma_oracle as so
import ssim_oracle as ss
import test_gpu_aniso_smoothing as GA
import test_gpu_smooth_sigma as GS
import test_gpu_ssim as GM
import tile_plan_cases as tp

pytestmark = pytest.mark.gpu

SIGMA = 1.3                     # dsigma: every tap of every radius is far above underflow
SIGMA_T, SIGMA_S = 1.3, 2.0     # aniso
SSIM_SIGMA = 1.5

def _lib():
    from kccotgan_amd import _lib
    return _lib


def _sid(shape):
    return "x".join(map(str, shape))


@pytest.fixture(scope="module")
def worst():
    w = {}
    yield w
    print("\nworst error / bound per family over the cases of this module:")
    for k in sorted(w):
        print("    %-14s %.3e / %.3e = %.3f   (%s)" % ((k,) + w[k]))


def _report(worst, family, what, err, bound):
    """print, and keep the worst ratio of the family; err and bound in one unit"""
    ratio = err / bound
    print("%s %s: error %.3e  bound %.3e  ratio %.3f" % (family, what, err, bound, ratio))
    if family not in worst or ratio > worst[family][0] / worst[family][1]:
        worst[family] = (err, bound, ratio, what)
    return ratio


# ---- dsigma_tile ---------------------------------------------------------------------------------------------------------------
DS_CASES = [("R%d-NI%d" % k, v[0], k[0], v[1], ("inst", k)) for k, v in sorted(tp.DSIGMA_INST.items())] + \
           [("%s-%s" % k, v[0], v[1], k[1], ("regime", k[0])) for k, v in sorted(tp.DSIGMA_REGIME.items())]


@pytest.mark.parametrize("name,shape,r,form,what", DS_CASES, ids=["%s-%s-%s" % (c[0], c[3], _sid(c[1])) for c in DS_CASES])
def test_dsigma_tile_case_reaches_its_plan_and_meets_the_bound(name, shape, r, form, what, worst):
    p = _lib().smooth_dsigma_plan(shape, r, tp.FORM_FLAGS[form])
    if what[0] == "inst":
        assert (p["launches"], p["R"], p["NI"]) == (1,) + what[1], (name, shape, form, p)
    else:
        assert tp.smooth_regime(p, what[1], p["Hv"], p["Tv"], p["Wv"], p["Cv"]), (name, shape, form, p)
    x = GS._rand(shape, 61)
    out, mx = GS._forward(x, SIGMA, r, form)
    _, ds = so.fields(x, so.f32(SIGMA), r, form, False, True)
    fails = []
    # random: the older modules' upstream gradient.  aligned (gout = ds/dsigma itself, as in the older grid): the terms add up
    # coherently, |ref| >= 0.01 Y, so a wrong term at a fraction of the positions cannot hide in the cancellation of a sum over
    # millions of random signs -- the bound is relative to Y, the power of a random gout falls as 1 / sqrt(elements)
    for kind, g in (("random", GS._rand(shape, 62, normal=True)), ("aligned", ds.to(torch.float32))):
        got = float(GS._dsigma(x, g, out, mx, SIGMA, r, form))
        ref, y = so.dsigma_ref(x, g, out, mx, so.f32(SIGMA), r, form)
        assert y > 0 and abs(ref) > 0 and (kind == "random" or abs(ref) >= 0.01 * y), (kind, ref, y)
        tag = "%s %s %s <%d,%d> %s got %.9e ref %.9e" % (name, form, shape, p["R"], p["NI"], kind, got, ref)
        if _report(worst, "dsigma_tile", tag, abs(got - ref), GS.BOUND * y) > 1.0:
            fails.append((kind, got, ref, y))
    assert not fails, (name, fails)


# ---- aniso_tile ----------------------------------------------------------------------------------------------------------------
# (name, shape, rt, rs, causal, job, what), in the order of (shape, radii, causal) so that the jobs of one forward follow each other
AN_CASES = sorted([("RS%d-NI%d" % k[:2], v[0], v[1], k[0], v[2], k[2], ("inst", k)) for k, v in tp.ANISO_INST.items()] +
                  [("%s-%s" % k[:2], v[0], v[1], v[2], k[1] == "causal", k[2], ("regime", k[0])) for k, v in tp.ANISO_REGIME.items()],
                  key=lambda c: (c[1], c[2], c[3], c[4], tp.JOBS.index(c[5]), c[0]))


@functools.lru_cache(maxsize=1)
def _aniso_forward(shape, cfg):
    x = GA.video(shape, 12)
    g = GA.rand(shape, 13, normal=True)
    out, mx = GA.k_fwd(x, cfg)
    return x, g, out, mx


def _measured(fn, *a):
    """an older module's check: its figures are printed whether it passes or not"""
    try:
        return fn(*a)
    except AssertionError as e:
        print("FAILED %s: %s" % (fn.__name__, e.args))
        raise


@pytest.mark.parametrize("name,shape,rt,rs,causal,job,what", AN_CASES,
                         ids=["%s-%s-%s-%s" % (c[0], c[5], "causal" if c[4] else "sym", _sid(c[1])) for c in AN_CASES])
def test_aniso_tile_case_reaches_its_plan_and_meets_the_bound(name, shape, rt, rs, causal, job, what, worst):
    p = _lib().smooth_aniso_plan(shape, rt, rs, causal, job)
    if what[0] == "inst":
        assert (p["launches"], p["RS"], p["NI"], tp.JOBS[p["job"]]) == (1,) + what[1], (name, shape, p)
    else:
        assert tp.smooth_regime(p, what[1], *shape[1:]), (name, shape, p)
    cfg = (SIGMA_T, SIGMA_S, rt, rs, causal)
    x, g, out, mx = _aniso_forward(shape, cfg)
    tag = "%s %s %s %s <%d,%d>" % (name, job, "causal" if causal else "sym", shape, p["RS"], p["NI"])
    if job == "fwd":
        err = _measured(GA.check_forward, x, out, mx, cfg)
        _report(worst, "aniso fwd", tag, err, GA.FWD_TOL)
    elif job == "adj":
        din = GA.k_bwd(g, out, mx, cfg)
        rel = _measured(GA.check_backward, g, out, mx, din, cfg)
        _report(worst, "aniso adj", tag, rel, GA.BWD_TOL)
    else:
        # the module's random gout, then one aligned with each derivative field (see the dsigma_tile test): both components are
        # held to the bound each time, the aligned one is then at least 0.01 Y
        _, gt, gs = ao.fields(x, so.f32(SIGMA_T), so.f32(SIGMA_S), rt, rs, causal, False, True)
        for kind, gk in (("random", g), ("aligned_t", gt.to(torch.float32))) + ((("aligned_s", gs.to(torch.float32)),) if rs else ()):
            got = GA.k_dsigma(x, gk, out, mx, cfg)
            r_t, r_s = _measured(GA.check_dsigma, x, gk, out, mx, got, cfg)
            _report(worst, "aniso dsigma_t", tag + " " + kind, r_t, GA.DS_BOUND)
            _report(worst, "aniso dsigma_s", tag + " " + kind, r_s, GA.DS_BOUND)
            assert float(got[0]) != 0.0 and (rs == 0 or float(got[1]) != 0.0)
            if kind != "random":
                refs, ys = ao.dsigma_ref(x, gk, out, mx, so.f32(SIGMA_T), so.f32(SIGMA_S), rt, rs, causal)
                k = 0 if kind == "aligned_t" else 1
                assert abs(refs[k]) >= 0.01 * ys[k], (kind, refs, ys)


# ---- ssim_walk -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,shape,r,reg_f,reg_b", tp.SSIM_CASES, ids=["%s-%s" % (c[0], _sid(c[1])) for c in tp.SSIM_CASES])
def test_ssim_walk_case_reaches_its_regimes_and_meets_the_bounds(name, shape, r, reg_f, reg_b, worst):
    L = _lib()
    win = 2 * r + 1
    for bwd, regs in ((0, reg_f), (1, reg_b)):
        p, one = L.ssim_plan(shape, r, bwd), L.ssim_plan((1,) + shape[1:], r, bwd)
        for reg in regs:
            assert tp.ssim_regime(p, reg, shape, r, bwd, one), (name, bwd, reg, p)
    kinds = ("noise", "flat") if "radius" in reg_f else ("noise",)
    fails = []
    for kind in kinds:
        x, y = GM.data(kind, shape, 71)
        g = ss.upstream(shape, 72, GM.DEV)
        xd, yd = x.double(), y.double()
        s, m = GM.k_fwd(x, y, win, SSIM_SIGMA)
        e_s = float((s.double() - ss.scores(xd, yd, SSIM_SIGMA, r)).abs().max())
        m_ref = ss.mse(xd, yd)
        e_m = float(((m.double() - m_ref).abs() / m_ref).max())
        tag = "%s %s r %d %s" % (name, shape, r, kind)
        figures = [("ssim " + kind, e_s, GM.TOL_SSIM[kind]), ("ssim mse", e_m, GM.TOL_MSE)]
        if kind == "noise" or r > 0:        # (the flat adjoint at radius 0: left out, see the module docstring)
            dy = GM.k_bwd(g, x, y, win, SSIM_SIGMA)
            ref = ss.adjoint(g.double(), xd, yd, SSIM_SIGMA, r)
            e_d = float((dy.double() - ref).abs().max()) / float(ref.abs().max())
            figures.append(("ssim dy " + kind, e_d, GM.TOL_DY if kind == "noise" else ss.CAP_DY))
        for family, err, bound in figures:
            if _report(worst, family, tag, err, bound) > 1.0:
                fails.append((family, tag, err, bound))
    assert not fails, fails
