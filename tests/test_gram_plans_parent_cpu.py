"""CPU tier: the host-only queries of the cost paths answer what they answered before the Gram paths' shared tail moved into
csrc/gram_tail.h and the choice of the path into one selector (gram_split, cost.hip).

tests/golden/gram_plans_parent.json was recorded by tests/golden/make_gram_plans_golden.py on a build of the commit before that
move; this module recomputes all of it through the same function (no GPU: none of the queries makes a device call) and asks
for ZERO differences over the full grid: the workspace sizes, the span of the fp64 Gram sums (return code, byte offset, number
of doubles) and the three row-block queries, under the default options and under each of cost_tile256=0, cost_tiled=0,
gram_f32=1 and cost_blocked=0.  The file holds one SHA-256 per (options, B) over every number of that row (12 K x 3 row
counts) and the landmark rows in full, which are compared field by field.  The all-reducing caller reads the workspace at
the span the query reports, so a span that moves is a wrong read, not an error.  A deliberate re-tuning of a planner or of
the dispatch re-records the file."""
import importlib.util
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GRID_FIELDS = ("cost3_workspace_bytes", "span_rc", "span_offset", "span_doubles", "cost_workspace_bytes")


@pytest.fixture(scope="module")
def both():
    spec = importlib.util.spec_from_file_location("make_gram_plans_golden", os.path.join(HERE, "golden", "make_gram_plans_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk, json.load(open(mk.PATH)), mk.compute()


def test_the_recording_covers_the_sweep(both):
    mk, want, got = both
    bs = [b for b in range(1, 1025) if b <= 64 or b % 32 == 0] + [2048, 4096, 4224]
    ks = [4, 252, 256, 260, 2560, 2596, 122880, 368640, 2359296, 2 ** 22, 2 ** 22 + 4, 2 ** 23]
    assert want["B"] == bs == mk.BS and want["K"] == ks == mk.KS and want["row_counts"] == [16, 32, 64] == mk.ROWS
    assert want["options"] == ["defaults", "cost_tile256=0", "cost_tiled=0", "gram_f32=1", "cost_blocked=0"] == got["options"]
    assert list(want["sha256"]) == want["options"] and all(list(t) == [str(b) for b in bs] for t in want["sha256"].values())
    assert len(got["grid"]) == len(got["rows"]) == 5 * len(bs) and len(got["counts"]) == len(bs)
    assert all(len(v) == len(ks) for v in got["grid"].values()) and all(len(v) == len(ks) and len(v[0]) == 3 for v in got["rows"].values())
    assert want["notes"] == {}                              # no entry had to be re-recorded: the two copies of the dispatch agreed
    # the landmarks the issue of the move quotes
    k = ks.index(2560)
    assert want["landmarks"]["defaults B=256"]["grid"][k][2:4] == [12582912, 196608]
    assert want["landmarks"]["cost_tile256=0 B=256"]["grid"][k][2:4] == [52428800, 163840]


def test_every_row_of_the_sweep_hashes_to_the_parents(both):
    """workspace sizes, the span of the Gram sums and the row-block queries: every (options, B) row, every K and row count"""
    mk, want, got = both
    now = mk.digest(got)["sha256"]
    diffs = ["%s B=%s: grid %s rows %s" % (o, b, got["grid"]["%s B=%s" % (o, b)], got["rows"]["%s B=%s" % (o, b)])
             for o, t in want["sha256"].items() for b, h in t.items() if now[o][b] != h]
    assert not diffs, (len(diffs), diffs[:3])
    # on top of the hashes: every path that has a Gram-sum split is in the grid, shapes without one report an empty span, and
    # the row-block form is supported somewhere, refused somewhere, and the refusal follows the options
    k = mk.KS.index(2560)
    assert all(tuple(got["grid"]["defaults B=%d" % b][k][2:4]) != (0, 0) for b in (1, 33, 64, 128, 256, 384))
    assert got["grid"]["defaults B=96"][k][2:4] == [0, 0] and got["grid"]["cost_tiled=0 B=256"][k][2:4] == [0, 0]
    assert got["rows"]["defaults B=256"][k][1][0] == 1 and got["rows"]["defaults B=256"][k][0][0] == 0
    assert got["rows"]["gram_f32=1 B=256"][k][1][0] == 0 and got["rows"]["defaults B=256"][k][1][1] == got["rows"]["gram_f32=1 B=256"][k][1][1] > 0


def test_the_landmark_rows_are_the_parents_field_by_field(both):
    mk, want, got = both
    assert sorted(want["landmarks"]) == sorted(mk.LANDMARKS)
    diffs = ["%s K=%d: %s %d -> %d" % (key, K, f, a, b) for key, w in want["landmarks"].items()
             for K, wk, gk in zip(mk.KS, w["grid"], got["grid"][key]) for f, a, b in zip(GRID_FIELDS, wk, gk) if a != b]
    diffs += ["%s K=%d rows=%d: %s -> %s" % (key, K, m, a, b) for key, w in want["landmarks"].items()
              for K, wk, gk in zip(mk.KS, w["rows"], got["rows"][key]) for m, a, b in zip(mk.ROWS, wk, gk) if a != b]
    assert not diffs, diffs[:20]


def test_the_shared_tail_stands_once_in_the_sources():
    """the chunk loop, the loss's distance block, the stacked finalize's descriptor and the name TilePlan: one occurrence each
    under csrc/ (the chunk sum and the distances in gram_tail.h), and the dispatch and the span query ask the one selector"""
    csrc = os.path.join(os.path.dirname(HERE), "kccotgan_amd", "csrc")
    texts = {n: open(os.path.join(csrc, n)).read() for n in sorted(os.listdir(csrc)) if n.endswith((".hip", ".h"))}
    for needle, home in (("for (; c + 8 <= nchunk; c += 8)", "gram_tail.h"), ("const double dyy = diag ? 0.0 :", "gram_tail.h"),
                         ("const double dxy = dxx + e_jj - 2.0 * (x_ij - x_jj);", "gram_tail.h"), ("struct StackFin {", "gram_tail.h"),
                         ("void gram_stack_finalize(", "gram_tail.h"), ("struct TilePlan {", "tile_walk.h"),
                         ("GramSplit gram_split(int B, int64_t K) {", "cost.hip")):
        assert [n for n, t in texts.items() for _ in range(t.count(needle))] == [home], needle
    assert texts["cost.hip"].count("gram_split(") == 3          # its definition, run_cost, kccot_pairwise_cost3_gram_sums_span
    for gone in ("TileFin", "Q256Fin", "gram_tile_finalize", "gram_q256_finalize", "void gram_sums_span(", "gram_q256_sums_span", "gram_tiled_sums_span",
                 "gram_q256_applies"):
        assert not [n for n, t in texts.items() if gone in t], gone
