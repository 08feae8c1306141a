"""CPU tier: the three host-only plan queries (kccot_smooth_dsigma_plan, kccot_smooth_aniso_plan, kccot_ssim_plan) and the case
table of tests/tile_plan_cases.py that is built on them.  No GPU: the queries run the planners of the launches on the host.

(a) every case of the table reaches, through the queries, exactly the instantiation or the regime it is listed for;
(b) every instantiation that the launch switches can name and the constexpr limits ds_max_ni / an_max_ni admit is in the table
    or in UNREACHED (with the box that was searched for it); the restatement of the switches and limits in the table module is
    pinned to the text of the .hip sources;
(c) UNREACHED holds nothing that the planner picks at the BASELINE shapes configs[1..3] with the trainer's radius 3, for any
    form, job or causal setting.  As the table stands UNREACHED and WIDE are empty: no case lies outside the 4 M-element box;
(d) the finding the table answers, as a regression note.  Before it, by the REAL planner over every case of
    test_gpu_smooth_sigma.py and test_gpu_aniso_smoothing.py (OLDER_GRIDS, recomputed here):
        dsigma_tile   6 of 43 instantiations: NI = 1 at R = 1, 2, 3, 4, 7 and <1, 2> (R = 5 and 6 never ran, nor NI > 2)
        aniso_tile    18 of 72: NI = 1 at RS = 0, 1, 2, 3, 4, 7 for the three jobs (RS = 5 and 6 never ran, nor any NI > 1)
    while at BASELINE the planner picks dsigma NI in {1, 2, 4, 6, 8} and aniso NI in {2, 4, 8}: no tile kernel that training
    runs had been compared with a reference.  (A hand transcription of the planners had counted 5 of 43; the real figure
    stands.)  ssim_walk: radii 2, 4 and 6 never ran, no case had three column tiles, a channel tile below min(C, 16), or took the
    branch that stops cutting H.

The queries themselves: the argument checks of the entry points with the same codes, a dsigma call that launches nothing says
so, and each planner rule exists once in the sources."""
import ctypes
import importlib.util
import os
import re

import pytest

import tile_plan_cases as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kccotgan_amd", "csrc")


def _L():
    from kccotgan_amd import _lib
    return _lib


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def ds_plan(shape, r, form):
    return _L().smooth_dsigma_plan(shape, r, tp.FORM_FLAGS[form])


# ---- (a) ------------------------------------------------------------------------------------------------------------------------
def test_every_dsigma_case_reaches_its_instantiation_or_regime():
    for (R, NI), (shape, form) in tp.DSIGMA_INST.items():
        p = ds_plan(shape, R, form)
        assert (p["launches"], p["R"], p["NI"]) == (1, R, NI), ((R, NI), shape, form, p)
        assert tp.dsigma_worthwhile(shape, R, form) and tp.dsigma_allowed(shape, R, form)
        assert tp.elems(shape) <= tp.MAX_ELEMS or (R, NI) in tp.WIDE["dsigma"]
        # the grid is the product of the pieces, in the kernel's view
        assert p["grid"] == p["Bv"] * p["nseg"] * p["ntt"] * p["ntw"] * p["ntc"]
        assert p["Bv"] * p["Hv"] * p["Tv"] * p["Wv"] * p["Cv"] == tp.elems(shape)
    for (regime, form), (shape, r) in tp.DSIGMA_REGIME.items():
        p = ds_plan(shape, r, form)
        assert tp.smooth_regime(p, regime, p["Hv"], p["Tv"], p["Wv"], p["Cv"]), (regime, form, shape, p)
    want = set((g, f) for g in tp.SMOOTH_REGIMES for f in (tp.FORMS if g == "NI>1" else ("THW", "causalTHW")))
    assert set(tp.DSIGMA_REGIME) == want


def test_every_aniso_case_reaches_its_instantiation_or_regime():
    L = _L()
    for (RS, NI, job), (shape, rt, causal) in tp.ANISO_INST.items():
        p = L.smooth_aniso_plan(shape, rt, RS, causal, job)
        assert (p["launches"], p["RS"], p["NI"], p["job"]) == (1, RS, NI, L.ANISO_JOBS[job]), ((RS, NI, job), shape, p)
        assert tp.aniso_worthwhile(shape, rt, RS, causal) and rt == tp.ANISO_RT
        assert tp.elems(shape) <= tp.MAX_ELEMS or (RS, NI, job) in tp.WIDE["aniso"]
        assert p["grid"] == shape[0] * p["nseg"] * p["ntt"] * p["ntw"] * p["ntc"]
    for (regime, tform, job), (shape, rt, rs) in tp.ANISO_REGIME.items():
        p = L.smooth_aniso_plan(shape, rt, rs, tform == "causal", job)
        assert tp.smooth_regime(p, regime, *shape[1:]), (regime, tform, job, shape, p)
    assert set(tp.ANISO_REGIME) == set((g, t, j) for g in tp.SMOOTH_REGIMES for t in ("sym", "causal") for j in tp.JOBS)
    # both T stencils among the instantiation cases with NI > 1
    assert set(c for (_, ni, _), (_, _, c) in tp.ANISO_INST.items() if ni > 1) == {False, True}


def test_every_ssim_case_reaches_its_regimes_and_the_cases_cover_every_regime():
    L = _L()
    seen = {0: set(), 1: set()}
    radii = {0: set(), 1: set()}
    for name, shape, r, reg_f, reg_b in tp.SSIM_CASES:
        for bwd, regs in ((0, reg_f), (1, reg_b)):
            p = L.ssim_plan(shape, r, bwd)
            one = L.ssim_plan((1,) + shape[1:], r, bwd)
            for g in regs:
                assert tp.ssim_regime(p, g, shape, r, bwd, one), (name, bwd, g, p)
                seen[bwd].add(g)
                if g == "radius":
                    radii[bwd].add(r)
            assert p["grid"] == shape[0] * shape[2] * p["nseg"] * p["ntw"] * p["ntc"]
    assert radii[0] == radii[1] == set(range(8))
    assert seen[0] == {"radius", "ntw3", "noseg"} and seen[1] == {"radius", "ntw3", "noseg", "ct_cut"}
    # the figures the cases were chosen by
    assert (L.ssim_plan((1, 12, 1, 100, 8), 2, 0)["ntw"], L.ssim_plan((1, 12, 1, 100, 8), 2, 1)["ntw"]) == (3, 4)
    p = L.ssim_plan((1, 30, 1, 30, 20), 7, 1)
    assert (p["ct"], p["ntc"]) == (8, 3)
    # forward, the channel tile is never narrower than min(C, 16): here and over a sweep of widths and radii
    for W in (30, 64, 100, 257, 1000):
        for C in (3, 12, 16, 20, 40):
            for r in range(8):
                if 2 * r < W:
                    assert L.ssim_plan((1, 30, 1, W, C), r, 0)["ct"] == min(C, 16), (W, C, r)


# ---- (b) ------------------------------------------------------------------------------------------------------------------------
def test_the_table_and_unreached_cover_every_nameable_instantiation():
    for fam, inst, nameable in (("dsigma", tp.DSIGMA_INST, tp.dsigma_nameable()), ("aniso", tp.ANISO_INST, tp.aniso_nameable())):
        un = tp.UNREACHED[fam]
        assert not set(inst) & set(un), fam
        assert set(inst) | set(un) == set(nameable), (fam, sorted(set(nameable) - set(inst) - set(un)))
        for key, box in un.items():
            assert isinstance(box, str) and "BOX" in box, (key, box)       # each entry carries the box that was searched
        assert set(tp.WIDE[fam]) <= set(inst)
    assert len(tp.dsigma_nameable()) == 43 and len(tp.aniso_nameable()) == 72


def test_the_restated_switches_and_limits_are_those_of_the_sources():
    sig, ani, ssim = _src("smooth_sigma.hip"), _src("smooth_aniso.hip"), _src("ssim.hip")
    assert "constexpr int ds_max_ni(int radius) { return radius <= 3 ? 8 : (radius == 4 ? 6 : (radius == 5 ? 5 : 4)); }" in sig
    assert ("constexpr int an_max_ni(int rs, int job) { return job == JOB_FWD ? (rs <= 3 ? 8 : 4) : (rs <= 1 ? 8 : (rs <= 3 ? 4 : 2)); }"
            in ani)
    ints = lambda pat, text: sorted(set(int(v) for v in re.findall(pat, text)))
    assert ints(r"launch_tile_ni<R, (\d+)>\(pl", sig) == list(tp.DS_NIS)
    assert ints(r"rc = launch_tile<(\d+)>\(pl", sig) == list(tp.DS_RADII)
    assert ints(r"launch_tile_ni<RS, (\d+)>\(job", ani) == list(tp.AN_NIS)
    assert ints(r"return launch_tile_rs<(\d+)>\(job", ani) == list(tp.AN_RADII)
    assert ints(r"return ss_launch_r<(\d+)>\(bwd", ssim) == list(range(8))
    # the switches refuse what the limits do not admit, at compile time
    assert "if constexpr (NI > ds_max_ni(R)) return fail(" in sig and "if constexpr (NI > an_max_ni(RS, JOB)) return fail(" in ani
    for r in tp.DS_RADII:
        assert tp.ds_max_ni(r) == {1: 8, 2: 8, 3: 8, 4: 6, 5: 5, 6: 4, 7: 4}[r]


def test_each_planner_rule_exists_once_and_the_queries_call_it():
    texts = {n: _src(n) for n in os.listdir(CSRC) if n.endswith((".hip", ".h"))}
    count = lambda needle: sum(t.count(needle) for t in texts.values())
    for needle in ("DsShape ds_shape(", "TilePlan tile_plan(", "TileGeom tile_geometry(", "TileSearch ds_search(", "TileSearch an_search(",
                   "int64_t tile_largest_grid(", "SsPlan ss_plan(", "constexpr int ds_max_ni(", "constexpr int an_max_ni("):
        assert count(needle) == 1, needle
    # the cost model of the two smoothing planners stands in the sources once (csrc/tile_walk.h), and both files search through it
    assert count("ragged * idle") == 1 and count("const double strided") == 1
    assert "ragged * idle" in texts["tile_walk.h"] and "const double strided" in texts["tile_walk.h"]
    assert "tile_plan(" in texts["smooth_sigma.hip"] and "tile_plan(" in texts["smooth_aniso.hip"]

    def body(text, name):
        start = text.index('extern "C" int %s(' % name)
        return text[start:text.index('\nextern "C"', start + 1)]

    q = body(texts["smooth_sigma.hip"], "kccot_smooth_dsigma_plan")
    e = body(texts["smooth_sigma.hip"] + '\nextern "C"', "kccot_smooth_dsigma_f32")
    for call in ("ds_check_flags(", "ds_check_dims(", "ds_check_size(", "ds_launches(", "ds_shape(", "ds_search(s, radius)", "tile_plan(q)",
                 "tile_geometry(q, pl)"):
        assert call in q and call in e, call
    q = body(texts["smooth_aniso.hip"], "kccot_smooth_aniso_plan")
    for call in ("an_check(", "an_allowed(", "an_check_fwd_flags(", "an_check_size(", "an_dsigma_launches(", "an_search_of(c, job)", "tile_plan(q)",
                 "tile_geometry(q, pl)"):
        assert call in q, call
    walk = texts["smooth_aniso.hip"]
    walk = walk[walk.index("int an_walk("):walk.index("int an_bwd(")]
    assert "an_search_of(c, job)" in walk and "tile_plan(q)" in walk and "a.g = tile_geometry(q, pl)" in walk
    q = body(texts["ssim.hip"], "kccot_ssim_plan")
    for call in ("ss_check(", "ss_plan(", "ss_check_index("):
        assert call in q, call
    # no transcription of a planner outside the library: the cost model's two landmarks appear in no Python file
    for top in ("kccotgan_amd", "tests", "tools"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, top)):
            for f in files:
                if f.endswith(".py") and f != os.path.basename(__file__):
                    text = open(os.path.join(dirpath, f)).read()
                    assert "strided" not in text or "ragged * idle" not in text, f


# ---- (c) ------------------------------------------------------------------------------------------------------------------------
def test_unreached_holds_nothing_the_planner_picks_at_baseline():
    L = _L()
    r = tp.BASELINE_RADIUS
    ds, an = set(), set()
    for name, shape in tp.BASELINE.items():
        for form in tp.FORMS:
            ds.add((r, ds_plan(shape, r, form)["NI"]))
        for causal in (False, True):
            for job in tp.JOBS:
                an.add((r, L.smooth_aniso_plan(shape, r, r, causal, job)["NI"], job))
    assert sorted(ds) == tp.BASELINE_PICKS["dsigma"] and sorted(an) == tp.BASELINE_PICKS["aniso"]
    assert not ds & set(tp.UNREACHED["dsigma"]) and not an & set(tp.UNREACHED["aniso"])
    assert ds <= set(tp.DSIGMA_INST) and an <= set(tp.ANISO_INST)
    # what training runs is NI > 1: the figures of the finding (module docstring)
    cfg1 = tp.BASELINE["cfg1"]
    assert [ds_plan(cfg1, r, f)["NI"] for f in ("T", "causalT", "THW", "causalTHW")] == [8, 8, 4, 2]
    assert all(ds_plan(tp.BASELINE[c], r, f)["NI"] == 6 for c in ("cfg2", "cfg3") for f in ("THW", "causalTHW"))
    assert [L.smooth_aniso_plan(cfg1, r, r, False, j)["NI"] for j in tp.JOBS] == [4, 4, 4]
    assert [L.smooth_aniso_plan(cfg1, r, r, True, j)["NI"] for j in tp.JOBS] == [2, 2, 2]
    for c in ("cfg2", "cfg3"):
        assert [L.smooth_aniso_plan(tp.BASELINE[c], r, r, False, j)["NI"] for j in tp.JOBS] == [8, 4, 4]
    # a wide case, if the table ever holds one, stays inside its BASELINE shape
    big = tp.BASELINE["cfg3"]
    for fam, inst in (("dsigma", tp.DSIGMA_INST), ("aniso", tp.ANISO_INST)):
        for key in tp.WIDE[fam]:
            assert all(a <= b for a, b in zip(inst[key][0], big)), key


# ---- (d) ------------------------------------------------------------------------------------------------------------------------
def test_the_older_grids_reach_what_the_docstring_says():
    spec = importlib.util.spec_from_file_location("find_tile_plan_cases", os.path.join(ROOT, "tools", "find_tile_plan_cases.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    old = tool.older_grids()
    assert old == tp.OLDER_GRIDS
    assert (len(old["dsigma"]["reached"]), old["dsigma"]["nameable"]) == (6, 43)
    assert old["dsigma"]["reached"] == [(1, 1), (1, 2), (2, 1), (3, 1), (4, 1), (7, 1)]
    assert (len(old["aniso"]["reached"]), old["aniso"]["nameable"]) == (18, 72)
    assert set(k[1] for k in old["aniso"]["reached"]) == {1} and set(k[0] for k in old["aniso"]["reached"]) == {0, 1, 2, 3, 4, 7}
    so = __import__("ssim_oracle")
    # ssim: the grid's radii, and 3 in test_another_data_range_scales_the_constants (win_size 7): 2, 4 and 6 never ran
    assert sorted(set(win // 2 for _, win, _, _ in so.GRID)) == [0, 1, 5, 7]


# ---- the queries -----------------------------------------------------------------------------------------------------------------
def test_a_dsigma_call_that_launches_no_tile_kernel_says_so():
    L = _L()
    for shape, r, flags in (((2, 8, 9, 8, 1), 0, 7), ((2, 8, 9, 8, 1), 3, 0), ((2, 8, 9, 8, 1), 0, 0)):
        p = L.smooth_dsigma_plan(shape, r, flags)
        assert p["launches"] == 0 and not any(p.values()), p
    assert L.smooth_dsigma_plan((2, 8, 9, 8, 1), 3, 7)["launches"] == 1
    # the anisotropic dsigma with both radii 0; the forward and the adjoint always launch
    assert not any(L.smooth_aniso_plan((2, 8, 9, 8, 1), 0, 0, False, "dsigma").values())
    assert L.smooth_aniso_plan((2, 8, 9, 8, 1), 0, 0, False, "fwd")["launches"] == 1
    assert L.smooth_aniso_plan((2, 8, 9, 8, 1), 0, 0, True, "adj")["launches"] == 1
    assert L.smooth_aniso_plan((2, 8, 9, 8, 1), 2, 0, False, "dsigma")["launches"] == 1


def test_the_plans_follow_the_merges_of_ds_shape():
    p = ds_plan((3, 8, 9, 5, 2), 3, "T")            # neither W nor H smoothed: W into C, B into H
    assert (p["Bv"], p["Hv"], p["Tv"], p["Wv"], p["Cv"]) == (1, 24, 9, 1, 10) and p["wt"] == 1 and p["ntw"] == 1
    p = ds_plan((3, 8, 9, 5, 2), 3, "HW")
    assert (p["Bv"], p["Hv"], p["Tv"], p["Wv"], p["Cv"]) == (3, 8, 9, 5, 2)
    p = ds_plan((3, 8, 9, 5, 2), 3, "causalTHW")
    assert (p["Bv"], p["Hv"], p["Tv"], p["Wv"], p["Cv"]) == (3, 8, 9, 5, 2)


def test_the_queries_apply_the_entry_points_argument_checks_with_the_same_codes():
    L = _L()
    lib = L.lib
    one, two, far, big = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 40), 1 << 40    # never dereferenced
    out = (ctypes.c_int * 32)()
    good = (2, 8, 9, 8, 1)
    # dsigma: (shape, radius, flags)
    bad = [(good, 3, 16), (good, 3, 32), (good, 3, 64), (good, 3, 128), (good, 3, 256), (good, 3, 8), (good, 3, 8 | 2), (good, 8, 7),
           (good, -1, 7), (good, 9, 1), (good, 8, 2), ((2, 8, 9, 3, 1), 3, 4)] + \
          [(tuple(0 if k == j else v for k, v in enumerate(good)), 3, 7) for j in range(5)]
    for shape, r, flags in bad:
        rc_q = lib.kccot_smooth_dsigma_plan(*shape, r, flags, out)
        msg_q = lib.kccot_last_error().split(b": ", 1)[1]
        rc_e = lib.kccot_smooth_dsigma_f32(one, one, one, one, None, *shape, 1.3, r, flags, one, one, big, None)
        assert rc_q == rc_e == L.EINVAL and msg_q == lib.kccot_last_error().split(b": ", 1)[1], (shape, r, flags)
    assert lib.kccot_smooth_dsigma_plan(*good, 3, 7, None) == L.EINVAL and b"null" in lib.kccot_last_error()
    assert lib.kccot_smooth_dsigma_plan(*good, 9, 1 | 8, out) == L.EINVAL        # (radius 9 is out of range even for a causal T)
    assert lib.kccot_smooth_dsigma_plan(*good, 7, 1 | 8, out) == 0 and lib.kccot_smooth_dsigma_plan(2, 8, 3, 8, 1, 7, 1 | 8, out) == 0
    assert lib.kccot_smooth_dsigma_plan(1 << 15, 1 << 15, 1 << 15, 1, 1, 3, 1, out) == L.EUNSUPPORTED
    assert b"too large" in lib.kccot_last_error()

    # aniso: (shape, radius_t, radius_s, flags) per job
    def entry(job, shape, rt, rs, flags):
        if job == 0:
            return lib.kccot_smooth_aniso_fwd_f32(one, *shape, 1.3, rt, 2.0, rs, flags, two, one, one, big, None)
        if job == 1:
            return lib.kccot_smooth_aniso_bwd_f32(one, one, one, *shape, 1.3, rt, 2.0, rs, flags, one, one, big, None)
        return lib.kccot_smooth_aniso_dsigma_f32(one, one, one, one, None, *shape, 1.3, rt, 2.0, rs, flags, one, one, big, None)

    bad = [(good, 3, 3, 1), (good, 3, 3, 2), (good, 3, 3, 4), (good, 3, 3, 512), (good, 8, 3, 0), (good, 3, 8, 0), (good, -1, 3, 0),
           (good, 9, 3, 0), ((2, 8, 3, 8, 1), 3, 3, 0), ((2, 3, 9, 8, 1), 3, 3, 0), ((2, 8, 9, 3, 1), 3, 3, 0), (good, 3, 3, 16 | 32)] + \
          [(tuple(0 if k == j else v for k, v in enumerate(good)), 3, 3, 0) for j in range(5)]
    for job in (0, 1, 2):
        for shape, rt, rs, flags in bad:
            rc_q = lib.kccot_smooth_aniso_plan(*shape, rt, rs, flags, job, out)
            msg_q = lib.kccot_last_error().split(b": ", 1)[1]
            assert rc_q == entry(job, shape, rt, rs, flags) == L.EINVAL, (job, shape, rt, rs, flags)
            assert msg_q == lib.kccot_last_error().split(b": ", 1)[1], (job, shape, rt, rs, flags)
        assert lib.kccot_smooth_aniso_plan(2, 8, 3, 8, 1, 7, 3, 8, job, out) == 0          # a causal T takes any radius_t
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, 0, job, None) == L.EINVAL and b"null" in lib.kccot_last_error()
    # the protocol bits: where the job's entry points take them
    for flags in (16, 32):
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, flags, 0, out) == 0
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, flags, 1, out) == L.EINVAL == entry(1, good, 3, 3, flags)
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, flags, 2, out) == L.EINVAL == entry(2, good, 3, 3, flags)
    for flags in (64, 128):
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, flags, 0, out) == L.EINVAL == entry(0, good, 3, 3, flags)
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, flags, 1, out) == 0          # (the sharded backward)
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, flags, 2, out) == L.EINVAL == entry(2, good, 3, 3, flags)
    for job in (-1, 3):
        assert lib.kccot_smooth_aniso_plan(*good, 3, 3, 0, job, out) == L.EINVAL and b"job" in lib.kccot_last_error()
    assert lib.kccot_smooth_aniso_plan(1 << 15, 1 << 15, 1 << 15, 8, 1, 3, 3, 0, 0, out) == L.EUNSUPPORTED

    # ssim: (shape, radius)
    def ss_entry(bwd, shape, r):
        if bwd:
            return lib.kccot_ssim_bwd_f32(one, one, two, *shape, 1.5, r, 1.0, far, one, big, None)
        return lib.kccot_ssim_fwd_f32(one, two, *shape, 1.5, r, 1.0, one, one, one, big, None)

    good = (2, 16, 3, 16, 1)
    bad = [(good, 8), (good, -1), ((2, 10, 3, 16, 1), 5), ((2, 16, 3, 10, 1), 5), ((2, 1, 3, 16, 1), 1)] + \
          [(tuple(0 if k == j else v for k, v in enumerate(good)), 3) for j in range(5)]
    for bwd in (0, 1):
        for shape, r in bad:
            rc_q = lib.kccot_ssim_plan(*shape, r, bwd, out)
            msg_q = lib.kccot_last_error().split(b": ", 1)[1]
            assert rc_q == ss_entry(bwd, shape, r) == L.EINVAL and msg_q == lib.kccot_last_error().split(b": ", 1)[1], (bwd, shape, r)
        assert lib.kccot_ssim_plan(*good, 5, bwd, None) == L.EINVAL and b"null" in lib.kccot_last_error()
        assert lib.kccot_ssim_plan(2, 11, 3, 11, 1, 5, bwd, out) == 0                      # the 1 x 1 map
        assert lib.kccot_ssim_plan(1 << 20, 16, 1 << 12, 16, 1, 5, bwd, out) == L.EUNSUPPORTED and b"too large" in lib.kccot_last_error()


def test_the_wrappers_raise_as_the_package_does():
    L = _L()
    with pytest.raises(ValueError, match="radius"):
        L.smooth_dsigma_plan((2, 8, 9, 8, 1), 8, 7)
    with pytest.raises(ValueError, match="REFLECT"):
        L.smooth_aniso_plan((2, 3, 9, 8, 1), 3, 3, False, "adj")
    with pytest.raises(ValueError, match="does not fit"):
        L.ssim_plan((2, 10, 3, 16, 1), 5, True)
    with pytest.raises(NotImplementedError, match="too large"):
        L.ssim_plan((1 << 20, 16, 1 << 12, 16, 1), 5, False)
    assert (L.DSIGMA_PLAN_INTS, L.ANISO_PLAN_INTS, L.SSIM_PLAN_INTS) == (17, 13, 8)
    for header, name, n in (("kccot_smooth_sigma.h", "KCCOT_SMOOTH_DSIGMA_PLAN_INTS", 17), ("kccot_smooth_aniso.h", "KCCOT_SMOOTH_ANISO_PLAN_INTS", 13),
                            ("kccot_metrics.h", "KCCOT_SSIM_PLAN_INTS", 8)):
        assert "#define %s %d\n" % (name, n) in open(os.path.join(ROOT, "include", header)).read()
