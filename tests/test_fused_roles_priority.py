"""The wave priority of the reverse sweep of sinkhorn_fused_roles, held on the emitted gfx950 code (CPU: hipcc cross-compiles).

The two roles share every SIMD, and the SIMD's vector port goes to the higher priority, then to the older wave.  The role
that is on the dependent chain in a pass (gradient read -> multiplies -> serial adds -> DPP -> write) runs that pass at a
raised priority and is back at 0 in front of the barrier that ends it; the role that evaluates its plan runs at 0; the
forward loop, where the other role only waits at the barrier, runs at 0 throughout (sweep_prio, sinkhorn.hip).
Both roles raise (the form that measured best, profiles/sinkhorn_sweep_priority_ab.json), so in all 16 instances and in the
sweep loop of either role:

  1. an s_setprio with a non-zero operand lies between the barrier that opens the chain pass and the first ds_read behind it;
  2. an s_setprio 0 lies between the chain's ds_write_b32 and the next s_barrier, and these two are the loop's only ones;
  3. no forward loop (a loop, nested blocks included, that takes a logarithm and holds two barriers) contains an s_setprio;
  4. on every path to s_endpgm the last s_setprio executed is 0 (the kernel starts at 0): a data-flow pass over the blocks
     of the kernel, which also covers the sweep's peeled first iteration and the loop's exits.

The code of the parent commit holds no s_setprio at all: 1 and 2 fail on it."""
import re

import pytest

from test_abi import _device_isa
from test_fused_roles_schedule import EPT_LPR, _is_inst, _sweep_loops


@pytest.fixture(scope="module")
def roles_kernels(tmp_path_factory):
    kernels = _device_isa("sinkhorn.hip", tmp_path_factory.mktemp("isa"))
    roles = {k: v for k, v in kernels.items() if "sinkhorn_fused_roles" in k}
    assert len(roles) == 4 * len(EPT_LPR), sorted(roles)
    return roles


def _op(line):
    return line.split()[0]


def _blocks(body):
    """[(label or None, loop comment, [instruction, ...])] in layout order; the first block is the kernel's entry."""
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
            blocks[-1][2].append(line)
    return blocks


def _forward_loops(body):
    """[(header label, [instruction, ...])]: every loop, the blocks of its nested loops included, that contains v_log_f32 and
    at least two s_barrier -- the forward loop of either role (its block sums nest wave loops, so it is not innermost)."""
    blocks = _blocks(body)
    out = []
    for label, note, _ in blocks:
        if label is None or "Loop Header" not in note:
            continue
        name = label[2:]
        inner = {name} | {l[2:] for l, n, _ in blocks if l and ("Parent Loop %s " % name) in n + " "}
        ins = [x for l, n, b in blocks if (l and l[2:] in inner) or any(("Header=%s " % h) in n + " " for h in inner) for x in b]
        op = [_op(l) for l in ins]
        if any(o.startswith("v_log_f32") for o in op) and sum(o == "s_barrier" for o in op) >= 2:
            out.append((label, ins))
    return out


def test_the_chain_pass_of_either_role_runs_raised_and_ends_at_zero(roles_kernels):
    for name, body in roles_kernels.items():
        loops = _sweep_loops(body)
        assert len(loops) == 2, name
        for label, ins in loops:
            n = len(ins)
            prio = [(i, l.split()[1]) for i, l in enumerate(ins) if _op(l) == "s_setprio"]
            assert len(prio) == 2, (name, label, prio)
            w = next(i for i, l in enumerate(ins) if _op(l) == "ds_write_b32")
            back = next(k for k in range(1, n + 1) if _op(ins[(w - k) % n]) == "s_barrier")
            chain = [ins[(w - back + k) % n] for k in range(1, back)]              # behind the opening barrier, up to the write
            first_read = next(k for k, l in enumerate(chain) if l.startswith("ds_read"))
            raised = [l for l in chain[:first_read] if _op(l) == "s_setprio"]
            assert len(raised) == 1 and int(raised[0].split()[1]) != 0, (name, label, chain[:first_read + 1])
            fwd = next(k for k in range(1, n + 1) if _op(ins[(w + k) % n]) == "s_barrier")
            tail = [ins[(w + k) % n] for k in range(1, fwd)]                       # behind the write, up to the closing barrier
            assert [l.split()[1] for l in tail if _op(l) == "s_setprio"] == ["0"], (name, label, tail)


def test_no_forward_loop_changes_the_priority(roles_kernels):
    for name, body in roles_kernels.items():
        loops = _forward_loops(body)
        assert len(loops) >= 2, (name, [l for l, _ in loops])                     # the row role's and the column role's
        for label, ins in loops:
            assert not [l for l in ins if _op(l) == "s_setprio"], (name, label)


def test_the_priority_is_zero_on_every_path_to_the_end(roles_kernels):
    """States: the set of priorities a block can be entered with; the entry block starts at {0}.  A block leaves with the
    operand of its last s_setprio, or with what it was entered with.  Successors: the targets of its branches, and the next
    block in layout unless it ends in s_branch or s_endpgm."""
    for name, body in roles_kernels.items():
        blocks = _blocks(body)
        index = {label: k for k, (label, _, _) in enumerate(blocks) if label}
        assert not [l for _, _, b in blocks for l in b if _op(l) in ("s_setpc_b64", "s_swappc_b64")], name
        succ, last = [], []
        for k, (_, _, ins) in enumerate(blocks):
            s = [index[l.split()[1]] for l in ins if _op(l).startswith(("s_cbranch_", "s_branch"))]
            if not (ins and _op(ins[-1]) in ("s_branch", "s_endpgm")) and k + 1 < len(blocks):
                s.append(k + 1)
            succ.append(s)
            p = [l.split()[1] for l in ins if _op(l) == "s_setprio"]
            last.append(p[-1] if p else None)
        state = [set() for _ in blocks]
        state[0] = {"0"}
        work = [0]
        while work:
            k = work.pop()
            leaves = {last[k]} if last[k] is not None else state[k]
            for s in succ[k]:
                if not leaves <= state[s]:
                    state[s] |= leaves
                    work.append(s)
        ends = [k for k, (_, _, ins) in enumerate(blocks) if any(_op(l) == "s_endpgm" for l in ins)]
        assert ends, name
        for k in ends:
            leaves = {last[k]} if last[k] is not None else state[k]
            assert leaves == {"0"}, (name, blocks[k][0], leaves)
        assert sum(_op(l) == "s_setprio" for _, _, b in blocks for l in b) >= 4, name       # both roles, raise and drop
