#!/usr/bin/env python
"""Writes tests/golden/gram_plans_parent.json: what the host-only queries of the cost paths answer -- the workspace sizes, where
the fp64 Gram sums sit in the workspace (kccot_pairwise_cost3_gram_sums_span) and what the row-block form supports -- recorded
on a build of the commit BEFORE the Gram paths' shared tail moved into csrc/gram_tail.h and the choice of the path into one
selector.  tests/test_gram_plans_parent_cpu.py recomputes everything with compute() and compares: the move changes nothing
here.  A deliberate re-tuning of a planner or of the dispatch re-records the file:

    python tests/golden/make_gram_plans_golden.py

Host only: none of the queries makes a device call.  The sweep is a full grid, nothing is drawn.

compute() returns the tables; the file holds one SHA-256 per (options, B) over that row of all three (digest()), and the
rows of LANDMARKS in full:

    grid     one row per (options, B): for every K of KS the list
                 [kccot_pairwise_cost3_workspace_bytes, span rc, span byte offset, span doubles, kccot_pairwise_cost_workspace_bytes(B, B, K)]
    rows     one row per (options, B): for every K of KS and every row count of ROWS the pair
                 [kccot_pairwise_cost3_rows_gram_supported, kccot_pairwise_cost3_rows_gram_workspace_bytes]
    counts   one row per B: kccot_pairwise_cost3_rows_gram_sums_count at every row count of ROWS

`notes` names every entry that was re-recorded because the two copies of the dispatch disagreed at the parent (none did)."""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PATH = os.path.join(HERE, "gram_plans_parent.json")
BS = [b for b in range(1, 1025) if b <= 64 or b % 32 == 0] + [2048, 4096, 4224]
KS = [4, 252, 256, 260, 2560, 2596, 122880, 368640, 2359296, 1 << 22, (1 << 22) + 4, 1 << 23]
OPTIONS = [{}, {"cost_tile256": 0}, {"cost_tiled": 0}, {"gram_f32": 1}, {"cost_blocked": 0}]
ROWS = [16, 32, 64]
NOTES = {}
LANDMARKS = ["defaults B=64", "defaults B=128", "defaults B=256", "defaults B=384", "defaults B=512", "cost_tile256=0 B=256",
             "gram_f32=1 B=64"]


def opt_name(o):
    return ",".join("%s=%d" % kv for kv in sorted(o.items())) or "defaults"


def compute():
    from kccotgan_amd import _lib
    lib = _lib.lib
    off, cnt = ctypes.c_size_t(0), ctypes.c_size_t(0)
    grid, rows = {}, {}
    for o in OPTIONS:
        with _lib.options(**o):
            for B in BS:
                g, r = [], []
                for K in KS:
                    rc = lib.kccot_pairwise_cost3_gram_sums_span(B, K, ctypes.byref(off), ctypes.byref(cnt))
                    g.append([int(lib.kccot_pairwise_cost3_workspace_bytes(B, K)), int(rc), off.value, cnt.value,
                              int(lib.kccot_pairwise_cost_workspace_bytes(B, B, K))])
                    r.append([[int(lib.kccot_pairwise_cost3_rows_gram_supported(m, B, K)),
                               int(lib.kccot_pairwise_cost3_rows_gram_workspace_bytes(m, B, K))] for m in ROWS])
                grid["%s B=%d" % (opt_name(o), B)] = g
                rows["%s B=%d" % (opt_name(o), B)] = r
    counts = {"B=%d" % B: [int(lib.kccot_pairwise_cost3_rows_gram_sums_count(m, B)) for m in ROWS] for B in BS}
    return {"B": BS, "K": KS, "options": [opt_name(o) for o in OPTIONS], "row_counts": ROWS, "grid": grid, "rows": rows,
            "counts": counts, "notes": NOTES}


def digest(res):
    """what the file holds: {"sha256": {options: {B: hash of the row of grid, rows and counts}}, "landmarks": {key: the rows}}"""
    sha = {}
    for key in res["grid"]:
        o, b = key.split(" B=")
        text = json.dumps([res["grid"][key], res["rows"][key], res["counts"]["B=" + b]], separators=(",", ":"))
        sha.setdefault(o, {})[b] = hashlib.sha256(text.encode()).hexdigest()
    out = {k: res[k] for k in ("B", "K", "options", "row_counts", "notes")}
    out["sha256"] = sha
    out["landmarks"] = {k: {"grid": res["grid"][k], "rows": res["rows"][k]} for k in LANDMARKS}
    return out


if __name__ == "__main__":
    res = digest(compute())
    with open(PATH, "w") as f:          # one option setting / one landmark per line
        out = []
        for k in sorted(res):
            v = res[k]
            if k == "sha256":
                v = "{\n" + ",\n".join("  %s: %s" % (json.dumps(o), json.dumps(t, separators=(",", ":"))) for o, t in v.items()) + "\n}"
            elif k == "landmarks":
                v = "{\n" + ",\n".join("  %s: %s" % (json.dumps(a), json.dumps(v[a], separators=(",", ":"))) for a in v) + "\n}"
            else:
                v = json.dumps(v)
            out.append("%s: %s" % (json.dumps(k), v))
        f.write("{\n" + ",\n".join(out) + "\n}\n")
    assert json.load(open(PATH)) == res
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))
