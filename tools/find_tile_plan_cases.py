#!/usr/bin/env python
"""Finds the cases of tests/tile_plan_cases.py: for every instantiation of dsigma_tile<R, NI> and aniso_tile<RS, NI, JOB> that
the launch switches can name, the shape with the fewest elements that reaches it; for every tiling regime, the smallest shape
that lies in it.  Drives the host-only plan queries (kccot_smooth_dsigma_plan, kccot_smooth_aniso_plan) and nothing else: no
GPU, no copy of a planner rule.  The boxes, the regime predicates and the nameable sets are those of tests/tile_plan_cases.py.

    python tools/find_tile_plan_cases.py            # search, print the block
    python tools/find_tile_plan_cases.py --write    # and put it between the markers of tests/tile_plan_cases.py

About fifteen seconds on eight cores (one process per radius)."""
import argparse
import multiprocessing
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import tile_plan_cases as tp        # noqa: E402
from kccotgan_amd import _lib       # noqa: E402

BEGIN, END = "# ---- BEGIN GENERATED", "# ---- END GENERATED"


def ds_plan(shape, r, form):
    return _lib.smooth_dsigma_plan(shape, r, tp.FORM_FLAGS[form])


def an_plan(shape, rt, rs, causal, job):
    return _lib.smooth_aniso_plan(shape, rt, rs, causal, job)


# ---- instantiations: shapes in ascending size, so the first hit of a key is its smallest shape
def dsigma_radius(r):
    missing = set(k for k in tp.dsigma_nameable() if k[0] == r)
    found = {}
    for shape in tp.box_shapes(tp.BOX):
        for form in tp.FORMS[r % 5:] + tp.FORMS[:r % 5]:       # (of the forms that reach a key at one size, not always the same)
            if not tp.dsigma_worthwhile(shape, r, form):
                continue
            key = (r, ds_plan(shape, r, form)["NI"])
            if key in missing:
                missing.discard(key)
                found[key] = (shape, form)
        if not missing:
            break
    return found


def aniso_radius(rs):
    missing = set(k for k in tp.aniso_nameable() if k[0] == rs)
    found = {}
    for shape in tp.box_shapes(tp.BOX):
        for causal in ((True, False) if rs % 2 else (False, True)):     # (so that half the cases run the causal T)
            rt = tp.ANISO_RT
            if not tp.aniso_worthwhile(shape, rt, rs, causal):
                continue
            for job in tp.JOBS:
                p = an_plan(shape, rt, rs, causal, job)
                key = (rs, p["NI"], job)
                if p["launches"] and key in missing:
                    missing.discard(key)
                    found[key] = (shape, rt, causal)
        if not missing:
            break
    return found


# ---- what the planner picks at BASELINE with the trainer's radius, every form / job / causal setting
def baseline_picks():
    r = tp.BASELINE_RADIUS
    ds = set((r, ds_plan(s, r, f)["NI"]) for s in tp.BASELINE.values() for f in tp.FORMS)
    an = set((r, an_plan(s, r, r, c, j)["NI"], j) for s in tp.BASELINE.values() for c in (False, True) for j in tp.JOBS)
    return ds, an


def wide_search(ds_keys, an_keys):
    """the smallest shape of WIDE_BOX for the BASELINE picks that BOX did not reach"""
    r = tp.BASELINE_RADIUS
    ds, an = {}, {}
    for shape in tp.box_shapes(tp.WIDE_BOX, tp.elems(tp.BASELINE["cfg3"])):
        for form in tp.FORMS:
            key = (r, ds_plan(shape, r, form)["NI"])
            if key in ds_keys and key not in ds:
                ds[key] = (shape, form)
        for causal in (False, True):
            for job in tp.JOBS:
                key = (r, an_plan(shape, r, r, causal, job)["NI"], job)
                if key in an_keys and key not in an:
                    an[key] = (shape, r, causal)
        if len(ds) == len(ds_keys) and len(an) == len(an_keys):
            break
    return ds, an


# ---- regimes, at the trainer's radius
def regimes():
    r = tp.BASELINE_RADIUS
    shapes = {"NI>1": tp.box_shapes(tp.BOX)}
    rest = tp.box_shapes(tp.REGIME_BOX)
    ds, an = {}, {}
    for regime in tp.SMOOTH_REGIMES:
        for form in (tp.FORMS if regime == "NI>1" else ("THW", "causalTHW")):
            for shape in shapes.get(regime, rest):
                if not tp.dsigma_worthwhile(shape, r, form):
                    continue
                p = ds_plan(shape, r, form)
                if tp.smooth_regime(p, regime, p["Hv"], p["Tv"], p["Wv"], p["Cv"]):
                    ds[(regime, form)] = (shape, r)
                    break
        for causal in (False, True):
            for job in tp.JOBS:
                for shape in shapes.get(regime, rest):
                    if not tp.aniso_worthwhile(shape, r, r, causal):
                        continue
                    if tp.smooth_regime(an_plan(shape, r, r, causal, job), regime, *shape[1:]):
                        an[(regime, "causal" if causal else "sym", job)] = (shape, r, r)
                        break
    return ds, an


# ---- the finding this table answers: what the three older GPU modules reach, by the real planner
def older_grids():
    import test_gpu_aniso_smoothing as ta
    import test_gpu_smooth_sigma as ts
    ds = set()

    def add_ds(shape, r, forms=tp.FORMS, fallback=(1, 0)):
        for form in forms:
            q = max(x for x in (r,) + fallback if x <= r and tp.dsigma_allowed(shape, x, form))     # (as those tests lower r)
            p = ds_plan(shape, q, form)
            if p["launches"]:
                ds.add((p["R"], p["NI"]))

    for shape in ts.SHAPES:
        for r in ts.RADII:
            for form in tp.FORMS:
                if r and tp.dsigma_allowed(shape, r, form):
                    add_ds(shape, r, (form,))
    for shape, r in ts.TILED:
        add_ds(shape, r)
    for shape, r, _ in ts.GUARD_CASES:
        add_ds(shape, r, fallback=(3, 1, 0))
    for shape in ((2, 8, 9, 8, 1), (1, 8, 9, 8, 1), (2, 64, 30, 64, 1), (1, 64, 30, 64, 1), (2, 8, 9, 8, 2)):
        add_ds(shape, 3)
    for shape in ((2, 8, 9, 8, 1), (2, 64, 30, 64, 1)):         # the isotropic limit of test_gpu_aniso_smoothing.py
        for r in (3, 4):
            add_ds(shape, r, ("THW", "causalTHW"))
    an = set()

    def add_an(shape, rt, rs, jobs=tp.JOBS):
        for causal in (False, True):
            if tp.aniso_allowed(shape, rt, rs, causal):
                for job in jobs:
                    p = an_plan(shape, rt, rs, causal, job)
                    if p["launches"]:
                        an.add((p["RS"], p["NI"], job))

    for shape in ta.SHAPES:
        for rt, rs in ta.RADII + [(7, 2)]:
            add_an(shape, rt, rs)
    for shape, (rt, rs) in ta.TILED:
        add_an(shape, rt, rs)
    for shape, (rt, rs), _ in ta.GUARD_CASES:
        add_an(shape, rt, rs)
    for shape in ((2, 8, 9, 8, 1), (1, 8, 9, 8, 1), (2, 64, 30, 64, 1), (1, 64, 30, 64, 1), (2, 8, 9, 8, 2)):
        add_an(shape, 2, 3)
    for shape in ((2, 8, 9, 8, 1), (2, 64, 30, 64, 1)):
        for r in (3, 4):
            add_an(shape, r, r)
    add_an((2, 64, 6, 64, 1), 2, 3, ("fwd", "adj"))             # the trainer's iteration
    return {"dsigma": {"nameable": len(tp.dsigma_nameable()), "reached": sorted(ds)},
            "aniso": {"nameable": len(tp.aniso_nameable()), "reached": sorted(an)}}


def box_text(name):
    return "%s of tests/tile_plan_cases.py" % name


def block():
    with multiprocessing.Pool(min(8, os.cpu_count() or 2)) as pool:
        ds_parts = pool.map_async(dsigma_radius, tp.DS_RADII)
        an_parts = pool.map_async(aniso_radius, tp.AN_RADII)
        ds_inst = {k: v for part in ds_parts.get() for k, v in part.items()}
        an_inst = {k: v for part in an_parts.get() for k, v in part.items()}
    ds_base, an_base = baseline_picks()
    ds_wide, an_wide = wide_search(ds_base - set(ds_inst), an_base - set(an_inst))
    ds_inst.update(ds_wide)
    an_inst.update(an_wide)
    ds_reg, an_reg = regimes()
    unreached = {"dsigma": {k: box_text("BOX") for k in tp.dsigma_nameable() if k not in ds_inst},
                 "aniso": {k: box_text("BOX") for k in tp.aniso_nameable() if k not in an_inst}}
    lines = [BEGIN + " (tools/find_tile_plan_cases.py --write)"]

    def table(name, d, comment):
        lines.append("# " + comment)
        lines.append("%s = {" % name)
        for k in sorted(d, key=lambda k: tuple(str(x) if isinstance(x, str) else x for x in k)):
            lines.append("    %r: %r," % (k, d[k]))
        lines.append("}")

    table("DSIGMA_INST", ds_inst, "(R, NI): (shape, form)")
    table("ANISO_INST", an_inst, "(RS, NI, job): (shape, radius_t, causal)")
    table("DSIGMA_REGIME", ds_reg, "(regime, form): (shape, radius)")
    table("ANISO_REGIME", an_reg, "(regime, T stencil, job): (shape, radius_t, radius_s)")
    lines.append("# the cases above that lie outside BOX: found in WIDE_BOX, for what the planner picks at BASELINE")
    lines.append("WIDE = %r" % {"dsigma": sorted(ds_wide), "aniso": sorted(an_wide)})
    lines.append("# what the planner picks at BASELINE (radius %d, every form / job / causal setting)" % tp.BASELINE_RADIUS)
    lines.append("BASELINE_PICKS = %r" % {"dsigma": sorted(ds_base), "aniso": sorted(an_base)})
    lines.append("# nameable, admitted by the constexpr limits, reached by no shape of the box searched for it")
    lines.append("UNREACHED = {")
    for fam in ("dsigma", "aniso"):
        lines.append("    %r: {" % fam)
        for k in sorted(unreached[fam], key=lambda k: tuple(str(x) if isinstance(x, str) else x for x in k)):
            lines.append("        %r: %r," % (k, unreached[fam][k]))
        lines.append("    },")
    lines.append("}")
    lines.append("# the instantiations that the cases of test_gpu_smooth_sigma.py and test_gpu_aniso_smoothing.py reach, by the real")
    lines.append("# planner: what the suite held to fp64 before this table")
    lines.append("OLDER_GRIDS = %r" % older_grids())
    lines.append(END)
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--write", action="store_true", help="replace the generated block of tests/tile_plan_cases.py")
    args = ap.parse_args()
    text = block()
    if not args.write:
        sys.stdout.write(text)
        return
    path = os.path.join(ROOT, "tests", "tile_plan_cases.py")
    src = open(path).read()
    head, tail = src[:src.index(BEGIN)], src[src.index(END) + len(END) + 1:]
    open(path, "w").write(head + text + tail)
    print("wrote %s" % path)


if __name__ == "__main__":
    main()
