"""CPU tier: the tile planners and the workspace sizes answer what they answered before the planners moved into csrc/tile_walk.h.

tests/golden/tile_walk_parent.json was recorded by tests/golden/make_tile_walk_golden.py on a build of the commit before that
move; this module recomputes all of it through the same function (the host-only plan queries and the two *_workspace_bytes
calls: no GPU) and asks for ZERO differences: every plan int of every case of tests/tile_plan_cases.py and of the BASELINE shapes at
the radii 0..7 (a difference is reported with the name of the field), both workspace sizes, and one SHA-256 per (family,
radius, job) over a seeded sweep of 4000 further tuples.  A deliberate re-tuning of a planner re-records the file."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def both():
    spec = importlib.util.spec_from_file_location("make_tile_walk_golden", os.path.join(HERE, "golden", "make_tile_walk_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk, json.load(open(mk.PATH)), mk.compute()


@pytest.mark.parametrize("block", ["cases", "baseline"])
def test_every_plan_int_is_the_parents(both, block):
    mk, want, got = both
    assert sorted(want[block]) == sorted(got[block])
    diffs = []
    for key, w in want[block].items():
        fields = mk.DS_FIELDS if key.startswith("dsigma") else mk.AN_FIELDS
        assert len(w) == len(got[block][key]) == len(fields)
        diffs += ["%s: %s %d -> %d" % (key, f, a, b) for f, a, b in zip(fields, w, got[block][key]) if a != b]
    assert not diffs, diffs
    assert len(want["cases"]) == 43 + 13 + 72 + 30 and len(want["baseline"]) == 3 * 8 * (5 + 6)


def test_both_workspace_sizes_are_the_parents(both):
    mk, want, got = both
    assert sorted(want["workspace"]) == sorted(got["workspace"]) and len(want["workspace"]) > mk.WS_SWEEP
    diffs = ["%s: %s %d -> %d" % (k, f, a, b) for k, w in want["workspace"].items()
             for f, a, b in zip(("dsigma", "aniso"), w, got["workspace"][k]) if a != b]
    assert not diffs, diffs


def test_the_seeded_sweep_hashes_to_the_parents(both):
    mk, want, got = both
    assert want["seed"] == got["seed"] == mk.SEED and want["sweep_counts"] == got["sweep_counts"]
    assert want["sweep_tuples"] == 2 * mk.N_SWEEP >= 3000
    assert want["coverage"] == got["coverage"] and all(v > 0 for v in want["coverage"].values())
    # every radius of either family, every job
    assert set(want["sweep"]) == set(["dsigma r%d" % r for r in range(8)] + ["aniso rs%d %s" % (r, j) for r in range(8) for j in mk.tp.JOBS])
    diffs = [k for k in want["sweep"] if want["sweep"][k] != got["sweep"][k]]
    assert not diffs, diffs
