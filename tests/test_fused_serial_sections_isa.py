"""The serial sections of sinkhorn_fused_roles, held on the emitted gfx950 code (CPU: hipcc cross-compiles).

The launch is a chain of dependent half-steps on one CU per problem, so whatever stands between its two loops or behind them
is waited for by all 16 waves.  Neither place needs global memory for the result: the sweep takes g = w[p] from the kernel
arguments and nits from a register, the final cost is formed from the elements of C the prologue loaded, and dC is
transposed through LDS.  So, in all 16 instances and for either role, in the order the compiler laid the blocks out:

  1. between the end of the role's forward loop and the header of its sweep loop there is no global_atomic_*, no
     global_load_* and no s_waitcnt vmcnt(0) -- no cost hand-off, no re-read of C, no drain;
  2. behind the sweep loops the only global_load_dword are the three sc1 loads of the cost hand-off (the workgroup whose
     ticket came last reads the costs): dC is stored once per row and never read back.

A forward loop is a loop (nested blocks included) that takes a logarithm and holds two barriers, a sweep loop an innermost
loop with v_exp_f32, two barriers, a ds_write_b32 and no logarithm, as in test_fused_roles_priority.py and
test_fused_roles_schedule.py.  The parent commit fails both checks in every instance: the hand-off and the re-read stand
between the loops, and the column role adds to dC in global memory behind them."""
import re

import pytest

from test_abi import _device_isa
from test_fused_roles_schedule import EPT_LPR, _is_inst


@pytest.fixture(scope="module")
def roles_kernels(tmp_path_factory):
    kernels = _device_isa("sinkhorn.hip", tmp_path_factory.mktemp("isa"))
    roles = {k: v for k, v in kernels.items() if "sinkhorn_fused_roles" in k}
    assert len(roles) == 4 * len(EPT_LPR), sorted(roles)
    return roles


def _op(line):
    return line.split()[0]


def _blocks(body):
    """[(label or None, loop comment, [(position, instruction), ...])] in layout order; the first block is the entry."""
    blocks = [(None, "", [])]
    for i, line in enumerate(body):
        m = re.match(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)(.*)$", line)
        if m:
            note, j = m.group(2), i + 1
            while j < len(body) and body[j].startswith(";") and not body[j].startswith((";;#", "; %bb.")):
                note += " " + body[j]
                j += 1
            blocks.append((m.group(1), note, []))
        elif _is_inst(line):
            blocks[-1][2].append((i, line))
    return blocks


def _loops(body):
    """(forward loops, sweep loops), each [(first position, last position)] of the loop's instructions in the layout."""
    blocks = _blocks(body)
    fwd, sweep = [], []
    for label, note, _ in blocks:
        if label is None or "Loop Header" not in note:
            continue
        name = label[2:]
        inner = {name} | {l[2:] for l, n, _ in blocks if l and ("Parent Loop %s " % name) in n + " "}
        ins = [x for l, n, b in blocks if (l and l[2:] in inner) or any(("Header=%s " % h) in n + " " for h in inner) for x in b]
        op = [_op(l) for _, l in ins]
        span = (min(i for i, _ in ins), max(i for i, _ in ins))
        logs, bars = any(o.startswith("v_log_f32") for o in op), sum(o == "s_barrier" for o in op)
        if logs and bars >= 2:
            fwd.append(span)
        if ("This Inner Loop Header" in note and not logs and bars == 2 and any(o.startswith("v_exp_f32") for o in op)
                and any(o == "ds_write_b32" for o in op)):
            sweep.append(span)
    return fwd, sweep


def _sections(name, body):
    """[(end of the forward loop, start of the sweep loop, end of the sweep loop)] for the two roles.  With the shortcut a
    role's forward loop is found more than once (the loop and the loop around its jump): the one that ends last in front of
    the sweep loop bounds the stretch between the loops."""
    fwd, sweep = _loops(body)
    assert len(sweep) == 2 and len(fwd) >= 2, (name, fwd, sweep)
    sweep.sort()
    out = []
    for k, (s0, s1) in enumerate(sweep):
        lo = sweep[k - 1][1] if k else -1
        ends = [f1 for f0, f1 in fwd if lo < f0 and f1 < s0]
        assert ends, (name, "no forward loop in front of the sweep loop at", s0, fwd)
        out.append((max(ends), s0, s1))
    return out


def _behind(name, body, s1):
    """[(position, instruction)] behind the sweep loop that ends at s1, in layout order, up to the end of its role's code.
    The two roles are the arms of the kernel's first branch (the role is wave-uniform: s_cbranch_scc on the wave number), laid
    out one behind the other: the first arm ends where that branch's target begins, the second at the end of the kernel."""
    first = next(l for l in body if _is_inst(l) and _op(l).startswith("s_cbranch_"))
    assert _op(first).startswith("s_cbranch_scc"), (name, first)
    split = body.index(first.split()[1] + ":")
    fwd, sweep = _loops(body)
    assert min(s[1] for s in sweep) < split < max(s[0] for s in sweep), (name, split, sweep)    # one sweep loop in either arm
    end = split if s1 < split else len(body)
    return [(i, l) for i, l in enumerate(body) if s1 < i < end and _is_inst(l)]


def test_nothing_between_the_loops_touches_global_memory(roles_kernels):
    bad = []
    for name, body in roles_kernels.items():
        for f1, s0, _ in _sections(name, body):
            between = [l for l in body[f1 + 1:s0] if _is_inst(l)]
            assert any(_op(l) == "s_barrier" for l in between), (name, "the barrier in front of the sweep is not in the stretch")
            bad += [(name, l) for l in between
                    if _op(l).startswith(("global_atomic_", "global_load_")) or l.startswith("s_waitcnt vmcnt(0)")]
    assert not bad, bad[:8]


def test_the_tail_loads_nothing_but_the_hand_off(roles_kernels):
    for name, body in roles_kernels.items():
        tails = [_behind(name, body, s1) for _, _, s1 in _sections(name, body)]
        loads = [l for tail in tails for _, l in tail if _op(l).startswith("global_load_")]
        assert len(loads) == 3 and all(_op(l) == "global_load_dword" and l.endswith("sc1") for l in loads), (name, loads)
        # ... and the kernel's one returning atomic, which they follow, is behind a sweep loop too
        atomics = [i for i, l in enumerate(body) if _is_inst(l) and _op(l).startswith("global_atomic_")]
        assert len(atomics) == 1 and any(i == atomics[0] for tail in tails for i, _ in tail), (name, atomics)
