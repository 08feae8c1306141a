"""csrc/sigmoid_lstm.hip held to float64: kccot_sigmoid_lstm_{fwd,bwd}_f32 through the C ABI and through gan._SigmoidLSTM at the
trainer's own shape (B, T, U) = (64, 30, 8) and at the edges of the kernels.  Cases, inputs, oracle and yardstick are those of
tests/test_oracle_sigmoid_lstm.py, which proves the oracle on the CPU against float64 autograd of the module's own loop.

Every comparison is bounded by
    |kernel - ref| <= margin max(yardstick, 4 2^-24) max |ref|
with the yardstick the error of the CPU fp32 tensor-op loop on the same inputs and margin 8 (the figure of
tests/test_gpu_generator_cells_fp64.py for kernels whose summation order differs from the yardstick's: wh h is summed j = 0..U-1 by
fused multiply-adds here, by a GEMM there).  No element is masked.  Each test prints error and yardstick (-s).

Largest errors measured on an MI355X, as multiples of max(yardstick, 4 2^-24) max |ref| (the margin, 8, is the cap):
  C ABI (h_seq, c_seq, dgx)  0.68 at the trainer's (64,30,8); edges 0.80 at (5,6,16), 0.75 at (3,6,64), 0.71 at (67,7,8), 0.70 at
                             (1,30,8), 0.66 at (3,4,17), 0.63 at (1,1,1), 0.58 at (2,4,33), the rest 0.36 .. 0.62
  saturated, gx x 20         0.98, everything finite      misaligned 0.68 / 0.40 / 0.66, and the aligned call's bits
  module                     4.09 at (64,30,32,8): its dWx, a stock GEMM over 1 920 rows (yardstick 2.5e-7; the tensor-op loop on the
                             device measures 3.69 there); y, dx, db, dWh <= 2.2; 1.11 at (3,5,7,3), 1.07 at (67,2,5,16), 0.45 at
                             (2,1,4,64), where T = 1 leaves dWh exactly 0
  dWh of the Function        0.53
  launches per module call   exactly one sigmoid_lstm_fwd<8> and one sigmoid_lstm_bwd<8>
Kernel mutants, each tried once against this module (52 tests):
  gate order f, i, c, o in the backward   25 fail: every test with a gradient (all 16 ABI cases, saturated, the three
                                          misaligned cases, the four module cases, the Function)
  whT dg carry dropped                    22 fail: the same without the cases with T = 1 ((3,1,8), (1,1,1), module (2,1,4,64)),
                                          which have no carry
  dc f carry dropped                      22 fail: the same 22
One thing found while writing this module: gradients accumulated into leaf .grad by .backward() inside the capture, after an
eager run on the default stream, ended the process in the capture's end (host side).  The capture test follows
kccotgan_amd.graph.GraphedLossStep instead: warm-up on a side stream, torch.autograd.grad into the capture's own tensors.
"""
import numpy as np
import pytest
import torch

import test_oracle_sigmoid_lstm as S
from kccotgan_amd import gan

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32
PAD = 64                               # NaN-filled floats before and after every buffer handed to the library


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


class Buf:
    """A device tensor of `shape` inside a NaN-filled allocation: PAD floats of guard zone on either side, the first element
    `off` floats past a 16-byte boundary."""

    def __init__(self, shape, src=None, off=0):
        n = int(np.prod(shape))
        self.n, self.lo = n, PAD + off
        self.raw = torch.full((n + 2 * PAD + 4,), float("nan"), device=DEV, dtype=F32)
        assert self.raw.data_ptr() % 16 == 0
        self.t = self.raw[self.lo:self.lo + n].view(tuple(shape))
        if src is not None:
            self.t.copy_(src)
        assert self.t.data_ptr() % 16 == 4 * (off % 4) and self.t.is_contiguous()

    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool(torch.isnan(self.raw[:self.lo]).all()) and bool(torch.isnan(self.raw[self.lo + self.n:]).all())


def _call(L, name, *args):
    rc = getattr(L.lib, name)(*args)
    torch.cuda.synchronize()
    assert rc == 0, "%s returned %d: %s" % (name, rc, L.lib.kccot_last_error().decode())


def abi(L, t, off=0, save_c=True, bwd=True):
    """h_seq, c_seq, dgx through the C ABI; every buffer guarded; returns the Bufs."""
    B, T, U4 = t["gx"].shape
    U = U4 // 4
    gx, wh, dh = Buf(t["gx"].shape, t["gx"], off), Buf(t["wh"].shape, t["wh"], off), Buf(t["dh"].shape, t["dh"], off)
    out = {"h_seq": Buf((B, T, U), off=off), "c_seq": Buf((B, T, U), off=off), "dgx": Buf((B, T, U4), off=off)}
    _call(L, "kccot_sigmoid_lstm_fwd_f32", gx.ptr(), wh.ptr(), B, T, U, out["h_seq"].ptr(), out["c_seq"].ptr() if save_c else None, None)
    if bwd:
        _call(L, "kccot_sigmoid_lstm_bwd_f32", gx.ptr(), wh.ptr(), out["h_seq"].ptr(), out["c_seq"].ptr(), dh.ptr(), B, T, U,
              out["dgx"].ptr(), None)
    out["inputs"] = (gx, wh, dh)
    return out


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_abi(tag, got, shape, scale=1.0):
    ref, yard = S.reference(shape, scale)
    worst = max(S.within("%s %s" % (tag, k), got[k].t, ref[k], yard[k]) for k in S.ABI_OUTPUTS)
    print("WORST abi %s: %.2f x max(yardstick, floor) (margin %d)" % (tag, worst, S.MARGIN))


# ================================================================ raw ABI
@pytest.mark.parametrize("shape", S.CASES)
def test_abi_against_fp64(L, shape):
    check_abi("%s" % (shape,), abi(L, S.inputs(shape)), shape)


def test_abi_saturated_gates_stay_finite_and_within_the_bound(L):
    got = abi(L, S.inputs(S.SATURATED, 20.0))
    assert all(bool(torch.isfinite(got[k].t).all()) for k in S.ABI_OUTPUTS)
    check_abi("saturated %s x20" % (S.SATURATED,), got, S.SATURATED, 20.0)


@pytest.mark.parametrize("shape", [S.TRAINER, (5, 6, 3), (3, 4, 17)])
def test_abi_pointers_one_float_off_a_16_byte_boundary_give_the_same_bits(L, shape):
    t = S.inputs(shape)
    a, b = abi(L, t), abi(L, t, off=1)
    assert all(same_bits(a[k].t, b[k].t) for k in S.ABI_OUTPUTS)
    check_abi("misaligned %s" % (shape,), b, shape)


@pytest.mark.parametrize("U", [8, 3, 64])
def test_sample_independence_row_b_of_a_batch_of_67_equals_the_sample_alone(L, U):
    shape = (67, 3, U)
    t = S.inputs(shape, seed=2)
    full = abi(L, t)
    for b in (0, 7, 8, 41, 66):
        one = abi(L, {k: (v if k == "wh" else v[b:b + 1].contiguous()) for k, v in t.items()})
        assert all(same_bits(one[k].t[0], full[k].t[b]) for k in S.ABI_OUTPUTS), (U, b)


def test_two_runs_give_identical_bits(L):
    t = S.inputs(S.TRAINER)
    a, b = abi(L, t), abi(L, t)
    assert all(same_bits(a[k].t, b[k].t) for k in S.ABI_OUTPUTS)


@pytest.mark.parametrize("shape", S.EDGES)
def test_guard_zones_around_every_buffer_are_intact_after_each_call(L, shape):
    for off in (0, 1):
        got = abi(L, S.inputs(shape), off=off)
        for k in S.ABI_OUTPUTS:
            assert got[k].guards_intact(), "%s off=%d: guard zone of %s overwritten" % (shape, off, k)
            assert bool(torch.isfinite(got[k].t).all()), "%s: %s not fully written" % (shape, k)
        assert all(b.guards_intact() for b in got["inputs"])
        fwd_only = abi(L, S.inputs(shape), off=off, save_c=False, bwd=False)
        assert fwd_only["h_seq"].guards_intact()
        assert bool(torch.isnan(fwd_only["c_seq"].raw).all()) and bool(torch.isnan(fwd_only["dgx"].raw).all())


@pytest.mark.parametrize("shape", [S.TRAINER, (67, 2, 3), (2, 4, 33)])
def test_forward_without_c_seq_gives_the_saving_forwards_h_seq_bit_for_bit(L, shape):
    t = S.inputs(shape)
    assert same_bits(abi(L, t, save_c=False, bwd=False)["h_seq"].t, abi(L, t, bwd=False)["h_seq"].t)


# ================================================================ the module
def module_gpu(case):
    m, x, w, ref, yard = S.module_reference(case)
    got = S.module_run(m, x, w, device=DEV)
    torch.cuda.synchronize()
    return got, ref, yard


@pytest.mark.parametrize("case", S.MODULE_CASES)
def test_module_against_fp64(case):
    assert gan._SLSTM_HIP
    got, ref, yard = module_gpu(case)
    worst = max(S.within("module %s %s" % (case, k), got[k], ref[k], yard[k]) for k in S.MODULE_OUTPUTS)
    print("WORST module %s: %.2f x max(yardstick, floor) (margin %d)" % (case, worst, S.MARGIN))


def test_module_runs_the_kernels_of_the_abi(L):
    """y and the gradient of gx are the C ABI's bits on the module's own gx."""
    m, x, w = S.module_inputs((5, 6, 7, 3))
    m = m.to(DEV)
    gx = m.wx(x.to(DEV)).detach().requires_grad_(True)
    y = gan._SigmoidLSTMHIP.apply(gx, m.wh.weight)
    dgx, dwh = torch.autograd.grad((y * w.to(DEV)).sum(), (gx, m.wh.weight))
    raw = abi(L, {"gx": gx.detach().cpu(), "wh": m.wh.weight.detach().cpu(), "dh": w})
    assert same_bits(y.detach(), raw["h_seq"].t) and same_bits(dgx, raw["dgx"].t)
    ref = S.oracle(gx, m.wh.weight, w)
    S.within("function dwh", dwh, ref["dwh"], S.err_of(S.loop(gx, m.wh.weight, w)["dwh"], ref["dwh"]))


def test_module_under_no_grad_does_not_allocate_c_seq(monkeypatch):
    from kccotgan_amd import _lib
    m, x, w = S.module_inputs((3, 5, 7, 3))
    m, x = m.to(DEV), x.to(DEV)
    seen = []
    real = _lib.lib

    class Spy:
        def __getattr__(self, name):
            if name == "kccot_sigmoid_lstm_fwd_f32":
                return lambda *a: (seen.append(a[6]), real.kccot_sigmoid_lstm_fwd_f32(*a))[1]
            return getattr(real, name)

    monkeypatch.setattr(_lib, "lib", Spy())
    y1 = m(x)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        y0 = m(x)
    torch.cuda.synchronize()
    grown = torch.cuda.memory_allocated() - before
    assert seen[0] is not None and seen[1] is None, seen
    assert same_bits(y0, y1.detach())
    # gx [3,5,12] (freed on return) and h_seq [3,5,3]: one allocator block of 512 bytes stays, a c_seq would be a second one
    assert grown <= 512, grown


def test_switch_off_reproduces_the_loop_bit_for_bit(monkeypatch):
    case = S.MODULE_CASES[0]
    m, x, w = S.module_inputs(case)
    monkeypatch.setattr(gan, "_SLSTM_HIP", False)
    got = S.module_run(m, x, w, device=DEV)

    def parent_loop(self, x):                          # the forward of gan._SigmoidLSTM before the kernel existed
        B, T, _ = x.shape
        gx = self.wx(x)
        h = x.new_zeros(B, self.units)
        c = torch.zeros_like(h)
        outs = []
        for t in range(T):
            gi, gf, gc, go = torch.chunk(gx[:, t] + self.wh(h), 4, dim=1)
            c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.sigmoid(gc)
            h = torch.sigmoid(go) * torch.sigmoid(c)
            outs.append(h)
        return torch.stack(outs, dim=1)

    monkeypatch.setattr(gan._SigmoidLSTM, "forward", parent_loop)
    want = S.module_run(m, x, w, device=DEV)
    torch.cuda.synchronize()
    assert all(same_bits(got[k], want[k]) for k in S.MODULE_OUTPUTS)
    _, _, _, ref, yard = S.module_reference(case)
    for k in S.MODULE_OUTPUTS:                          # and the loop on the device is what the yardstick says it is
        S.within("loop on the device %s" % k, got[k], ref[k], yard[k])


def test_units_above_64_and_float64_take_the_loop():
    m, x, w = S.module_inputs((2, 3, 4, 65))
    got = S.module_run(m, x, w, device=DEV)
    ref = S.module_run(m, x, w, dtype=torch.float64)
    for k in S.MODULE_OUTPUTS:
        assert S.err_of(got[k], ref[k]) < 1e-5
    m, x, w = S.module_inputs((3, 5, 7, 3))
    dev64 = S.module_run(m, x, w, device=DEV, dtype=torch.float64)
    cpu64 = S.module_run(m, x, w, dtype=torch.float64)
    assert all(S.err_of(dev64[k], cpu64[k]) < 1e-13 for k in S.MODULE_OUTPUTS)


def _step(m, x, w):
    for p in m.parameters():
        p.grad = None
    x.grad = None
    y = m(x)
    (y * w).sum().backward()
    return y


def test_graph_capture_of_forward_and_backward_replays_to_the_eager_bits():
    """The pattern of kccotgan_amd.graph.GraphedLossStep: warm-up on a side stream, gradients by torch.autograd.grad into
    the capture's own tensors (no leaf .grad accumulation, whose nodes keep the stream they were first used on)."""
    m, x, w = S.module_inputs(S.MODULE_CASES[0])
    m, x, w = m.to(DEV), x.to(DEV).requires_grad_(True), w.to(DEV)
    one = torch.ones((), device=DEV)

    def fwd_bwd():
        y = m(x)
        return [y.detach()] + list(torch.autograd.grad((y * w).sum(), [x] + list(m.parameters()), grad_outputs=one))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            eager = [t.clone() for t in fwd_bwd()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = fwd_bwd()
    for _ in range(2):
        for t in static:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert all(same_bits(a, b) for a, b in zip(static, eager))


def test_one_forward_and_one_backward_kernel_per_module_call():
    from torch.profiler import ProfilerActivity, profile
    m, x, w = S.module_inputs(S.MODULE_CASES[0])
    m, x, w = m.to(DEV), x.to(DEV).requires_grad_(True), w.to(DEV)
    _step(m, x, w)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _step(m, x, w)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "sigmoid_lstm" in e.name]
    print("sigmoid_lstm kernels of one module call:", names)
    assert len([n for n in names if "sigmoid_lstm_fwd" in n]) == 1 and len([n for n in names if "sigmoid_lstm_bwd" in n]) == 1
    assert len(names) == 2
