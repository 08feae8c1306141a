"""The schedule of the reverse sweep of sinkhorn_fused_roles, held on the emitted gfx950 code (CPU: hipcc cross-compiles).

The role split pays only if the evaluation of a role's NEXT transport plan (history reads, subtracts, adds, v_exp_f32) runs
in the pass in which the OTHER role is on the dependent chain (gradient read -> multiplies -> serial adds -> DPP -> write),
i.e. in front of the barrier that separates the two passes.  lds_barrier() is an asm volatile with a memory clobber: it
holds memory operations in place, not register arithmetic, and the compiler once sank the column role's whole plan behind it,
to the head of the chain.  The sweep therefore pins the plan registers in front of the barrier (keep_in_regs, sinkhorn.hip),
and this file checks what came out, in all 16 instances and in the sweep loop of either role:

  1. walking the loop body cyclically from any v_exp_f32, an s_barrier is met before a ds_write_b32: no plan arithmetic
     between the barrier a chain pass starts at and the write it ends with;
  2. the first vector-memory or LDS instruction behind the barrier that opens the chain pass is the read of the gradients the
     pass waits for: a ds_read whose destination feeds a multiply of the chain.

Before the pins, check 1 failed in all 16 instances, each time in the column role's loop; check 2 held.

A sweep loop is an innermost loop that contains v_exp_f32, exactly two s_barrier and a ds_write_b32, and no v_log_f32 (the
forward loop of the instances without the shortcut has the first three as well; its half-step takes a logarithm, the sweep
takes none).  The loop body is read in the order the compiler laid its blocks out, starting at the loop header."""
import re

import pytest

from test_abi import _device_isa

EPT_LPR = [(1, 16), (2, 16), (16, 4), (8, 8)]


@pytest.fixture(scope="module")
def roles_kernels(tmp_path_factory):
    kernels = _device_isa("sinkhorn.hip", tmp_path_factory.mktemp("isa"))
    roles = {k: v for k, v in kernels.items() if "sinkhorn_fused_roles" in k}
    want = ["sinkhorn_fused_rolesILi%dELi%dELb%dELi%dEEE" % (e, l, sc, nprob)
            for e, l in EPT_LPR for sc in (0, 1) for nprob in (3, 4)]
    assert len(roles) == 16 and all(sum(w in k for k in roles) == 1 for w in want), sorted(roles)
    return roles


def _is_inst(line):
    return bool(line) and not line.startswith((";", ".")) and not re.match(r"^\S+:", line)


def _innermost_loops(body):
    """[(header label, [instruction, ...])] for every innermost loop of a kernel: the blocks that the compiler's own comments
    assign to the loop (`=>This Inner Loop Header`, `in Loop: Header=BBx_y`), in layout order, rotated to start at the header."""
    blocks = []                                                    # (label or None, start-line comment, [instructions])
    for i, line in enumerate(body):
        m = re.match(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)(.*)$", line)
        if m:
            note = m.group(2)
            j = i + 1
            while j < len(body) and body[j].startswith(";") and not body[j].startswith((";;#", "; %bb.")):
                note += " " + body[j]                              # nested loops: the header's comment runs over several lines
                j += 1
            blocks.append((m.group(1), note, []))
        elif blocks and _is_inst(line):
            blocks[-1][2].append(line)
    loops = []
    for k, (label, note, _) in enumerate(blocks):
        if label is None or "This Inner Loop Header" not in note:
            continue
        tag = "in Loop: Header=%s " % label[2:]
        member = [b for b in range(len(blocks)) if b == k or tag in blocks[b][1] + " "]
        order = [b for b in member if b >= k] + [b for b in member if b < k]
        loops.append((label, [ins for b in order for ins in blocks[b][2]]))
    return loops


def _sweep_loops(body):
    out = []
    for label, ins in _innermost_loops(body):
        op = [l.split()[0] for l in ins]
        if (any(o.startswith("v_exp_f32") for o in op) and sum(o == "s_barrier" for o in op) == 2
                and any(o == "ds_write_b32" for o in op) and not any(o.startswith("v_log_f32") for o in op)):
            out.append((label, ins))
    return out


def _regs(operand):
    """The VGPR numbers an operand names: v7 -> {7}, v[4:7] -> {4, 5, 6, 7}."""
    m = re.match(r"^v\[(\d+):(\d+)\]", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"^v(\d+)\b", operand)
    return {int(m.group(1))} if m else set()


def _operands(line):
    return [o.strip() for o in line.split(None, 1)[1].split(",")] if " " in line else []


def test_both_sweep_loops_are_found_in_every_instance(roles_kernels):
    for name, body in roles_kernels.items():
        loops = _sweep_loops(body)
        assert len(loops) == 2, (name, [l for l, _ in loops])          # the row role's and the column role's


def test_no_plan_arithmetic_between_a_chain_pass_barrier_and_its_write(roles_kernels):
    bad = []
    for name, body in roles_kernels.items():
        for label, ins in _sweep_loops(body):
            n = len(ins)
            for i, l in enumerate(ins):
                if not l.startswith("v_exp_f32"):
                    continue
                for k in range(1, n + 1):
                    o = ins[(i + k) % n].split()[0]
                    if o == "s_barrier":
                        break
                    if o == "ds_write_b32":
                        bad.append((name, label, i, l))
                        break
    assert not bad, "v_exp_f32 on the chain side of a barrier: %s" % sorted({(n, l) for n, l, _, _ in bad})


def test_the_chain_pass_opens_with_the_read_of_the_gradients(roles_kernels):
    for name, body in roles_kernels.items():
        for label, ins in _sweep_loops(body):
            n = len(ins)
            writes = [i for i, l in enumerate(ins) if l.split()[0] == "ds_write_b32"]
            assert len(writes) == 1, (name, label, writes)
            w = writes[0]
            back = next(k for k in range(1, n + 1) if ins[(w - k) % n].split()[0] == "s_barrier")
            chain = [ins[(w - back + k) % n] for k in range(1, back)]          # behind the opening barrier, up to the write
            mem = [k for k, l in enumerate(chain) if l.startswith(("ds_", "global_", "buffer_", "flat_", "scratch_"))]
            assert mem, (name, label)
            first = chain[mem[0]]
            assert first.startswith("ds_read"), (name, label, first)
            dst = _regs(_operands(first)[0])
            feeds = [l for l in chain[mem[0] + 1:] if l.startswith(("v_mul_f32", "v_pk_mul_f32"))
                     and any(dst & _regs(o) for o in _operands(l)[1:])]
            assert feeds, (name, label, first, "feeds no multiply of the chain")
