#!/usr/bin/env python3
"""Issue budget of the FORWARD loops of sinkhorn_fused_roles, counted on the emitted gfx950 code (CPU only: hipcc cross-compiles).

The sweep has tools/sweep_issue_budget.py; this is the same count for the forward loop, with the same compile, classes and issue
prices (transcendental 8 cycles; plain, packed and DPP vector ALU 4; every s_nop 4; LDS, scalar and branch instructions are
counted and priced 0: they do not take the vector port).

In the forward only ONE role works per half-step: the row role from the barrier that closed the iteration before to the
iteration's first barrier, the column role between the iteration's first and second barrier; the other role's waves wait.
Eight working waves are two per SIMD, so a SIMD's vector port is asked for twice the wave's issue cycles per half-step, and the workgroup waits for all of it.  Two stretches are printed per instance and role:

  iteration   the blocks of the loop that every iteration runs: the loop without its nested loops (the wave loops of the stop
              rule's block sum, the history fill of the shortcut's jump) and without the blocks of the stop rule and of the
              shortcut's jump, which are entered by a branch that L = Lmin and shortcut = off never take.  Where the compiler
              laid such a block out in line the count includes it and says so ("rare blocks in line").
  chain       the instructions between the barrier that opens the role's half-step and its ds_write_b32, the write of the new
              dual: the stretch the whole workgroup waits for.

usage: forward_issue_budget.py [--json] [--all] [extra hipcc flags, e.g. -DKCCOT_FWD_TRIM=0]
       without --all only the headline instance <8,8,false,3> is printed in full, the others as one line each"""
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from sweep_issue_budget import PRICE, budget, device_isa  # noqa: E402


def _op(line):
    return line.split()[0]


def forward_loops(body, ept=None):
    """[(header label, role, iteration instructions, chain instructions)] of a role kernel's two forward loops.

    A forward loop is a loop header (not innermost: the block sum nests wave loops) whose OWN blocks, nested loops left out,
    hold a v_log_f32 and at least two s_barrier.  Its own blocks are read in layout order from the header.  The half-step is
    the stretch around the v_log_f32: back to the nearest s_barrier (or to the header: the row role's half-step opens the
    iteration, the barrier that opens it is the one that closed the iteration before) and on to the first ds_write_b32."""
    from test_fused_roles_priority import _blocks
    blocks = _blocks(body)
    out = []
    for k, (label, note, _) in enumerate(blocks):
        if label is None or "This Loop Header" not in note:
            continue
        tag = "in Loop: Header=%s " % label[2:]
        member = [b for b in range(len(blocks)) if b == k or tag in blocks[b][1] + " "]
        order = [b for b in member if b >= k] + [b for b in member if b < k]
        ins = [x for b in order for x in blocks[b][2]]
        ops = [_op(l) for l in ins]
        if not any(o.startswith("v_log_f32") for o in ops) or ops.count("s_barrier") < 2:
            continue
        lg = next(i for i, o in enumerate(ops) if o.startswith("v_log_f32"))
        first_barrier = ops.index("s_barrier")
        role = "row" if lg < first_barrier else "column"
        start = max([i for i in range(lg) if ops[i] == "s_barrier"], default=-1) + 1
        write = next(i for i in range(lg, len(ops)) if ops[i] == "ds_write_b32")
        chain = ins[start:write + 1]
        # the stretch found is ONE half-step: one logarithm, as many exponentials as a lane has entries, no barrier inside
        cops = [_op(l) for l in chain]
        assert sum(o.startswith("v_log_f32") for o in cops) == 1 and "s_barrier" not in cops, (label, role)
        assert ept is None or sum(o.startswith("v_exp_f32") for o in cops) == ept, (label, role, ept)
        # every iteration: up to the second barrier behind the header and the scalar tests behind it; what follows a
        # ds_bpermute_b32 or a third barrier in line belongs to the stop rule's block sum
        barriers = [i for i, o in enumerate(ops) if o == "s_barrier"]
        rare = next((i for i in range(barriers[1] + 1, len(ops))
                     if ops[i] in ("ds_bpermute_b32", "s_barrier") or ops[i].startswith("ds_")), len(ops))
        # ... cut back to the branch that guards it, if there is one
        guard = max([i for i in range(barriers[1], rare) if ops[i].startswith("s_cbranch")], default=None)
        every = ins[:guard + 1] if guard is not None else ins[:rare]
        out.append((label, role, every, chain, guard is None and rare < len(ops)))
    return out


def main():
    args = sys.argv[1:]
    as_json, show_all = "--json" in args, "--all" in args
    flags = [a for a in args if a not in ("--json", "--all")]
    with tempfile.TemporaryDirectory() as tmp:
        kernels, registers = device_isa(tmp, flags)
    out = {}
    for name, body in sorted(kernels.items()):
        if "sinkhorn_fused_roles" not in name:
            continue
        m = re.search(r"rolesILi(\d+)ELi(\d+)ELb(\d)ELi(\d)", name)
        key = "<%s,%s,%s,%s>" % (m.group(1), m.group(2), "true" if m.group(3) == "1" else "false", m.group(4))
        entry = {"registers": registers[name], "forward": {}}
        for label, role, every, chain, inline_rare in forward_loops(body, int(m.group(1))):
            assert role not in entry["forward"], (name, role)
            entry["forward"][role] = {"header": label, "iteration": budget(every), "chain": budget(chain),
                                      "rare_blocks_in_line": inline_rare}
        assert sorted(entry["forward"]) == ["column", "row"], (name, sorted(entry["forward"]))
        # two working waves per SIMD in each half-step
        entry["port_cycles_per_iteration_at_2_working_waves_per_simd"] = 2 * sum(
            r["iteration"]["issue_cycles"] for r in entry["forward"].values())
        entry["chain_port_cycles_per_iteration_at_2_working_waves_per_simd"] = 2 * sum(
            r["chain"]["issue_cycles"] for r in entry["forward"].values())
        out[key] = entry
    if as_json:
        print(json.dumps(out, indent=1))
        return
    print("issue prices (cycles): %s" % PRICE)
    for key, e in out.items():
        r, f = e["registers"], e["forward"]
        print("%-16s %3d VGPRs  %d B scratch | chain instructions: row %d  column %d | chain issue cycles per wave: row %d  column %d | "
              "port per iteration: chain %d, whole iteration %d" % (
                  key, r.get("vgprs", -1), r.get("scratch_bytes", -1), f["row"]["chain"]["instructions"],
                  f["column"]["chain"]["instructions"], f["row"]["chain"]["issue_cycles"], f["column"]["chain"]["issue_cycles"],
                  e["chain_port_cycles_per_iteration_at_2_working_waves_per_simd"],
                  e["port_cycles_per_iteration_at_2_working_waves_per_simd"]))
        if show_all or key == "<8,8,false,3>":
            for role in ("row", "column"):
                for what in ("iteration", "chain"):
                    b = f[role][what]
                    c = b["by_class"]
                    print("    %-6s %-9s %-10s %3d instructions: plain %d  transcendental %d  packed %d  DPP %d  s_nop %d  LDS %d  scalar %d  "
                          "other %d -> %d issue cycles%s" % (
                              role, what, f[role]["header"], b["instructions"], c["plain"], c["transcendental"], c["packed"], c["dpp"],
                              c["s_nop"], c["lds"], c["scalar"], c["other"], b["issue_cycles"],
                              "  (rare blocks in line)" if what == "iteration" and f[role]["rare_blocks_in_line"] else ""))


if __name__ == "__main__":
    main()
