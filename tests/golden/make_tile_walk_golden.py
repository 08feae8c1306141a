#!/usr/bin/env python
"""Writes tests/golden/tile_walk_parent.json: what the two tile planners (csrc/tile_walk.h behind kccot_smooth_dsigma_plan and
kccot_smooth_aniso_plan) and the two workspace-size calls answer, recorded on a build of the commit BEFORE the planners moved
into one header.  tests/test_tile_walk_parent_cpu.py recomputes everything with compute() and compares: a refactoring of the
planners changes nothing here.  A deliberate re-tuning re-records the file (and tests/tile_plan_cases.py with it):

    python tests/golden/make_tile_walk_golden.py

Host only: the plan queries and the workspace sizes make no device call.  Deterministic: the sweep is drawn by SEED.

    cases       every plan int of every case of tile_plan_cases.DSIGMA_INST / DSIGMA_REGIME / ANISO_INST / ANISO_REGIME
    baseline    every plan int at the BASELINE shapes for every form / job / causal setting at the radii 0..7
    workspace   both workspace sizes at every shape of the two blocks above and at the first WS_SWEEP shapes of the sweep
    sweep       N_SWEEP shapes, one dsigma and one aniso tuple each, from the axis lengths of BOX and REGIME_BOX (at most
                4 M elements), as one SHA-256 per (family, radius, job) over the tuples and their plan ints; `coverage` counts
                the shapes with C > 16, with W*C odd, with T < radius under a causal T, and with each extent equal to 1."""
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import tile_plan_cases as tp        # noqa: E402

PATH = os.path.join(HERE, "tile_walk_parent.json")
SEED = 20261021
N_SWEEP = 2000
WS_SWEEP = 150
DS_FIELDS = ("launches", "R", "NI", "tt", "wt", "ct", "hs", "ntt", "ntw", "ntc", "nseg", "grid", "Bv", "Hv", "Tv", "Wv", "Cv")
AN_FIELDS = ("launches", "RS", "NI", "job", "tt", "wt", "ct", "hs", "ntt", "ntw", "ntc", "nseg", "grid")
RADII = tuple(range(8))


def _L():
    from kccotgan_amd import _lib
    return _lib


def ds_ints(shape, r, form):
    p = _L().smooth_dsigma_plan(shape, r, tp.FORM_FLAGS[form])
    return [p[k] for k in DS_FIELDS]


def an_ints(shape, rt, rs, causal, job):
    p = _L().smooth_aniso_plan(shape, rt, rs, causal, job)
    return [p[k] for k in AN_FIELDS]


def _sid(shape):
    return "x".join(map(str, shape))


def sweep_tuples():
    """[(shape, (r, form), (rt, rs, causal, job))]: every tuple passes the argument checks of its query"""
    rng = random.Random(SEED)
    axes = {k: sorted(set(tp.BOX[k]) | set(tp.REGIME_BOX[k])) for k in "BHTWC"}
    out = []
    while len(out) < N_SWEEP:
        shape = tuple(rng.choice(axes[k]) for k in "BHTWC")
        if rng.random() < 0.25:                 # short axes: an extent of 1, a T below the radius
            j = rng.randrange(5)
            shape = tuple(rng.choice((1, 1, 2, 3)) if k == j else v for k, v in enumerate(shape))
        if tp.elems(shape) > tp.MAX_ELEMS:
            continue
        ds = [(r, f) for r in RADII for f in tp.FORMS if tp.dsigma_allowed(shape, r, f)]
        an = [(rt, rs, c, j) for rt in RADII for rs in RADII for c in (False, True) for j in tp.JOBS if tp.aniso_allowed(shape, rt, rs, c)]
        out.append((shape, rng.choice(ds), rng.choice(an)))
    return out


def compute():
    L = _L()
    res = {"seed": SEED, "ds_fields": list(DS_FIELDS), "an_fields": list(AN_FIELDS)}
    shapes = []
    cases = {}
    for (R, NI), (shape, form) in sorted(tp.DSIGMA_INST.items()):
        cases["dsigma_inst %d %d %s %s" % (R, NI, form, _sid(shape))] = ds_ints(shape, R, form)
        shapes.append(shape)
    for (regime, form), (shape, r) in sorted(tp.DSIGMA_REGIME.items()):
        cases["dsigma_regime %s %s %d %s" % (regime, form, r, _sid(shape))] = ds_ints(shape, r, form)
        shapes.append(shape)
    for (RS, NI, job), (shape, rt, causal) in sorted(tp.ANISO_INST.items()):
        cases["aniso_inst %d %d %s %d %d %s" % (RS, NI, job, rt, causal, _sid(shape))] = an_ints(shape, rt, RS, causal, job)
        shapes.append(shape)
    for (regime, tform, job), (shape, rt, rs) in sorted(tp.ANISO_REGIME.items()):
        cases["aniso_regime %s %s %s %d %d %s" % (regime, tform, job, rt, rs, _sid(shape))] = an_ints(shape, rt, rs, tform == "causal", job)
        shapes.append(shape)
    res["cases"] = cases
    base = {}
    for name, shape in sorted(tp.BASELINE.items()):
        shapes.append(shape)
        for r in RADII:
            for form in tp.FORMS:
                base["dsigma %s %s %d" % (name, form, r)] = ds_ints(shape, r, form)
            for causal in (False, True):
                for job in tp.JOBS:
                    base["aniso %s %s %d %d" % (name, job, causal, r)] = an_ints(shape, r, r, causal, job)
    res["baseline"] = base
    sweep = sweep_tuples()
    groups, cover = {}, {"C>16": 0, "WC_odd": 0, "T<radius_causal": 0, "B=1": 0, "H=1": 0, "T=1": 0, "W=1": 0, "C=1": 0}
    for shape, (r, form), (rt, rs, causal, job) in sweep:
        B, H, T, W, C = shape
        cover["C>16"] += C > 16
        cover["WC_odd"] += (W * C) % 2
        cover["T<radius_causal"] += (form.startswith("causal") and T < r) + (causal and T < rt)
        for k, v in zip("BHTWC", shape):
            cover["%s=1" % k] += v == 1
        text = ",".join(map(str, shape + (r, tp.FORM_FLAGS[form]) + tuple(ds_ints(shape, r, form)))) + ";"
        groups.setdefault("dsigma r%d" % r, []).append(text)
        text = ",".join(map(str, shape + (rt, rs, int(causal)) + tuple(an_ints(shape, rt, rs, causal, job)))) + ";"
        groups.setdefault("aniso rs%d %s" % (rs, job), []).append(text)
    assert all(v > 0 for v in cover.values()), cover
    res["coverage"] = {k: int(v) for k, v in cover.items()}
    res["sweep_tuples"] = sum(len(v) for v in groups.values())
    res["sweep_counts"] = {k: len(v) for k, v in sorted(groups.items())}
    res["sweep"] = {k: hashlib.sha256("".join(v).encode()).hexdigest() for k, v in sorted(groups.items())}
    ws = {}
    for shape in sorted(set(shapes)) + [s for s, _, _ in sweep[:WS_SWEEP]]:
        ws[_sid(shape)] = [L.lib.kccot_smooth_dsigma_workspace_bytes(*shape), L.lib.kccot_smooth_aniso_workspace_bytes(*shape)]
    res["workspace"] = ws
    return res


if __name__ == "__main__":
    res = compute()
    with open(PATH, "w") as f:          # one entry of a table per line
        rows = []
        for k in sorted(res):
            v = res[k]
            if isinstance(v, dict):
                v = "{\n" + ",\n".join("  %s: %s" % (json.dumps(a), json.dumps(v[a])) for a in sorted(v)) + "\n}"
            else:
                v = json.dumps(v)
            rows.append("%s: %s" % (json.dumps(k), v))
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
    assert json.load(open(PATH)) == res
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
