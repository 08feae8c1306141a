"""The forward loop of sinkhorn_fused_roles, held on the emitted gfx950 code (CPU: hipcc cross-compiles).

tools/forward_issue_budget.py counts, per instance and role, the instructions between the barrier that opens the role's
half-step and the ds_write_b32 of its new dual: the stretch all 16 waves of the workgroup wait for, 200 times per solve at
L = 100.  tests/golden/forward_budget_parent.json holds that count, the VGPRs and the scratch of the commit before the forward
trims.  In all 16 instances:

  1. no scratch;
  2. no more VGPRs than that commit;
  3. for either role, no more instructions on that stretch than that commit."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def budgets():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "forward_issue_budget.py"), "--json"], check=True,
                         stdout=subprocess.PIPE, universal_newlines=True).stdout
    now = json.loads(out)
    with open(os.path.join(ROOT, "tests", "golden", "forward_budget_parent.json")) as f:
        before = json.load(f)["instances"]
    assert sorted(now) == sorted(before) and len(now) == 16, sorted(now)
    return now, before


def test_no_instance_gained_scratch(budgets):
    now, before = budgets
    for key, e in now.items():
        assert e["registers"]["scratch_bytes"] == 0 == before[key]["scratch_bytes"], key


def test_vgpr_counts_did_not_rise(budgets):
    now, before = budgets
    rose = {key: (before[key]["vgprs"], e["registers"]["vgprs"]) for key, e in now.items()
            if e["registers"]["vgprs"] > before[key]["vgprs"]}
    assert not rose, rose


def test_the_chain_of_either_role_is_no_longer_than_before(budgets):
    now, before = budgets
    longer = {}
    for key, e in now.items():
        for role in ("row", "column"):
            have, had = e["forward"][role]["chain"]["instructions"], before[key]["chain_instructions"][role]
            if have > had:
                longer[(key, role)] = (had, have)
    assert not longer, longer


def test_the_headline_instance_lost_what_the_trims_took(budgets):
    """<8,8,false,3>: both roles lose two s_nop of the DPP max and the three address instructions (5); the row role also the
    three of |du| (8)."""
    now, before = budgets
    lost = {role: before["<8,8,false,3>"]["chain_instructions"][role] - now["<8,8,false,3>"]["forward"][role]["chain"]["instructions"]
            for role in ("row", "column")}
    assert lost["row"] >= 8 and lost["column"] >= 5, lost


def test_every_other_kernel_of_the_file_keeps_its_scratch_and_its_sweep_loops():
    """tests/golden/sinkhorn_kernels_parent.json: VGPRs, scratch bytes and the opcode sequence (a hash and a length) of every sweep
    loop -- an innermost loop with a barrier and an exponential and no logarithm -- of all 84 kernels of sinkhorn.hip on the
    commit before the forward trims.  Every kernel has the scratch and the sweep loops it had (the helper-sharing rule of DESIGN
    4.4), and no more VGPRs: the role kernels, the one-role fused kernels and the two-launch forward and sweep kernels, weighted
    ones included."""
    import hashlib
    import tempfile
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sweep_issue_budget import device_isa
    from test_fused_roles_schedule import _innermost_loops
    with tempfile.TemporaryDirectory() as tmp:
        kernels, meta = device_isa(tmp, [])
    with open(os.path.join(ROOT, "tests", "golden", "sinkhorn_kernels_parent.json")) as f:
        before = json.load(f)
    assert sorted(kernels) == sorted(before) and len(before) == 84
    moved = {}
    for name, body in kernels.items():
        loops = []
        for _, ins in _innermost_loops(body):
            op = [l.split()[0] for l in ins]
            if "s_barrier" in op and any(o.startswith("v_exp_f32") for o in op) and not any(o.startswith("v_log_f32") for o in op):
                loops.append(hashlib.sha1(" ".join(op).encode()).hexdigest()[:16] + ":%d" % len(op))
        b = before[name]
        if loops != b["sweep_loops"] or meta[name]["scratch_bytes"] != b["scratch_bytes"] or meta[name]["vgprs"] > b["vgprs"]:
            moved[name] = (b, dict(meta[name], sweep_loops=loops))
    assert sum(bool(b["sweep_loops"]) for b in before.values()) == 58
    assert not moved, moved
