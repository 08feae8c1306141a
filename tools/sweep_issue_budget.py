#!/usr/bin/env python3
"""Issue budget of the loops of sinkhorn_fused_roles, counted on the emitted gfx950 code (CPU only: hipcc cross-compiles).

Compiles kccotgan_amd/csrc/sinkhorn.hip the way tests/test_abi.py::_device_isa does, finds the two sweep loops of every
instance with the loop finder of tests/test_fused_roles_schedule.py (and the forward loops with the one of
tests/test_fused_roles_priority.py: the loops that take a logarithm, their rarely run nested wave loops included), and prints per loop and role the instruction count by class and the issue cycles one wave asks of its SIMD's
vector port per iteration, at the issue prices measured for gfx950: transcendental 8 cycles; plain, packed and DPP vector
ALU 4; every s_nop 4 (the price of `s_nop 0`; a longer one is not cheaper).  LDS, scalar and branch instructions are counted
and priced 0: they do not take the vector port.  Four waves share a SIMD in the 1024-thread instances (two of each role), so
the port's load per iteration is twice the sum of the two roles.

The row role's loop is the one whose body opens with the chain (its ds_write_b32 lies in front of the first s_barrier behind
the loop header); the column role's opens with its plan.

usage: sweep_issue_budget.py [--json] [--all] [extra hipcc flags, e.g. -DKCCOT_SWEEP_PRIO=0]
       without --all only the headline instance <8,8,false,3> is printed in full, the others as one line each"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

PRICE = {"transcendental": 8, "plain": 4, "packed": 4, "dpp": 4, "s_nop": 4, "lds": 0, "scalar": 0, "other": 0}
TRANS = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32")


def classify(line):
    op = line.split()[0]
    if op == "s_nop":
        return "s_nop"
    if op.startswith(TRANS):
        return "transcendental"
    if op.startswith("v_pk_"):
        return "packed"
    if op.startswith("v_"):
        return "dpp" if ("_dpp" in op or "quad_perm" in line or "row_" in line) else "plain"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith("s_"):
        return "scalar"
    return "other"


def budget(ins):
    count = {k: 0 for k in PRICE}
    for l in ins:
        count[classify(l)] += 1
    adds = sum(l.split()[0].startswith(("v_add_f32", "v_sub_f32")) and classify(l) == "plain" for l in ins)
    return {"instructions": len(ins), "by_class": count, "plain_add_sub_f32": adds,
            "s_setprio": [l.split()[1] for l in ins if l.startswith("s_setprio")],
            "issue_cycles": sum(PRICE[k] * v for k, v in count.items())}


def role_of(ins):
    op = [l.split()[0] for l in ins]
    return "row" if op.index("ds_write_b32") < op.index("s_barrier") else "column"


def device_isa(tmp, flags):
    """tests/test_abi.py::_device_isa for sinkhorn.hip (the same command line, plus the extra flags of an experiment build);
    returns the kernels' bodies and, from the comment block behind each body, its registers, scratch and occupancy."""
    out = os.path.join(tmp, "sinkhorn.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S"] + flags +
                   ["-o", out, os.path.join(ROOT, "kccotgan_amd", "csrc", "sinkhorn.hip")], check=True, stderr=subprocess.DEVNULL)
    kernels, meta, cur, body, done = {}, {}, None, [], None
    for line in open(out):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body, done = m.group(1), [], None
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                kernels[cur], cur, done = body, None, cur
                meta[done] = {}
            else:
                body.append(line.strip())
        elif done is not None:
            for tag, field in (("; NumVgprs:", "vgprs"), ("; ScratchSize:", "scratch_bytes"), ("; Occupancy:", "occupancy")):
                if line.startswith(tag):
                    meta[done][field] = int(line.split(":")[1])
    return kernels, meta


def main():
    from test_fused_roles_priority import _forward_loops
    from test_fused_roles_schedule import _sweep_loops
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
        entry = {"registers": registers[name], "sweep": {}, "forward": []}
        for label, ins in _sweep_loops(body):
            entry["sweep"][role_of(ins)] = dict(budget(ins), header=label)
        for label, ins in _forward_loops(body):
            entry["forward"].append(dict(budget(ins), header=label))
        assert sorted(entry["sweep"]) == ["column", "row"], (name, sorted(entry["sweep"]))
        entry["sweep_port_cycles_per_iteration_at_4_waves_per_simd"] = 2 * sum(r["issue_cycles"] for r in entry["sweep"].values())
        out[key] = entry
    if as_json:
        print(json.dumps(out, indent=1))
        return
    print("issue prices (cycles): %s" % PRICE)
    for key, e in out.items():
        full = show_all or key == "<8,8,false,3>"
        r = e["registers"]
        print("%-16s %3d VGPRs  %d B scratch  occupancy %d | sweep issue cycles per wave: row %d  column %d | port per iteration %d%s" % (
            key, r.get("vgprs", -1), r.get("scratch_bytes", -1), r.get("occupancy", -1), e["sweep"]["row"]["issue_cycles"],
            e["sweep"]["column"]["issue_cycles"], e["sweep_port_cycles_per_iteration_at_4_waves_per_simd"],
            "" if e["forward"] else " | no forward loop found"))
        if full:
            rows = [("sweep " + k, v) for k, v in sorted(e["sweep"].items())] + [("forward", v) for v in e["forward"]]
            for what, b in rows:
                c = b["by_class"]
                print("    %-13s %-10s %3d instructions: plain %d (f32 add/sub %d)  transcendental %d  packed %d  DPP %d  s_nop %d  LDS %d  "
                      "scalar %d  other %d -> %d issue cycles; s_setprio %s" % (
                          what, b["header"], b["instructions"], c["plain"], b["plain_add_sub_f32"], c["transcendental"], c["packed"],
                          c["dpp"], c["s_nop"], c["lds"], c["scalar"], c["other"], b["issue_cycles"], b["s_setprio"] or "none"))


if __name__ == "__main__":
    main()
