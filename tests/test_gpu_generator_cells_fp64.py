"""csrc/convlstm.hip and csrc/layernorm.hip held to float64: kccot_convlstm_cell_{fwd,bwd}_f32 and
kccot_channel_layernorm_{fwd,bwd}_f32 at the generator's own layer shapes and at the edges of both kernels.  Cases, inputs,
oracles and yardsticks are those of tests/test_oracle_generator_cells.py, which proves on the CPU what this module relies on
(the oracles against float64 autograd, the clamp decisions of the oracle against the fp32 hard_sigmoid, the chunk arithmetic).

Every comparison is bounded by
    |kernel - ref| <= margin max(yardstick, 4 2^-24) max |ref|
with the yardstick the error of the CPU fp32 tensor-op implementation on the same inputs (gan._cell_torch; nn.LayerNorm on the
permuted tensor) and margin 4 for the cell (elementwise: the device's tanhf and one rounding more or less), 8 for LayerNorm
(C channels summed sequentially, the parameter gradients in a block tree) and 8 for the ConvLSTM2D layer.  No element is masked
anywhere; a reference that is exactly zero everywhere demands exact zeros.  Each test prints error and yardstick (-s).

Largest errors measured on an MI355X (each test prints its figures, -s), as multiples of max(yardstick, 4 2^-24) max |ref| --
the margin is the cap -- with the kernels of the commit that adds this module (parent 5df9522):
  cell, generator shapes     0.48 (margin 4)      edges 0.76 at (1,5,3,3); misaligned 0.53, and the aligned call's bits
  cell, kinks                0.37; every gate gradient beyond a kink exactly 0, every one on or inside the bounds nonzero
  cell, gate bit for bit     equal on all 2048 values, 340 of which a fused multiply-add would round differently
  cell, absent upstreams     0.47; recurrence T = 12: 0.64; dg returned twice: each leaf .grad holds exactly 2 x the gradient
  LayerNorm, generator       1.72 at (8,256,4,4) (margin 8)      chunk cases 1.27 at (9,512,2,2), 1.26 at (11,256,4,4)
  LayerNorm, C = 2           1.32; offset 0.56 (y 2.8e-7, yardstick 6.3e-7); tiny 0.63; constant per pixel 0.49, rstd 0 ulp
  ConvLSTM2D layer           1.22 (margin 8): y 2.9e-7, dx 2.7e-7, parameter gradients <= 1.7e-7 of their largest value
Two things this module found in csrc/layernorm.hip, fixed in the same commit (figures of the parent's kernels first):
  constant per pixel, y      5.60e-5 -> 0 of max |ref| (29 x the bound; the CPU is exact here, so the floor applies): the rounding
                             of the sequential channel sum stayed in the mean, x - mean was pure rounding error and rstd = 31.6
                             scaled it up.  chan_ln_fwd now adds the mean of the residuals x - m0 from its second pass to m0.
                             The same correction took the offset case's y from 1.30e-6 to 2.78e-7.
  C = 1, dx                  3.54e-6 -> exactly 0: dy gamma was contracted into the difference dg - b as a fused multiply-add,
                             which left the product's rounding error, times rstd.  chan_ln_bwd_dx runs with contraction off.
Kernel mutants, each tried once: dhsig with exclusive bounds fails the kinks test; contraction on in convlstm.hip fails kinks,
gate-bit-for-bit and misaligned; per = N / nchunk in chan_ln_bwd_params fails the (11,256,4,4) and (9,512,2,2) chunk cases;
variance as E[x^2] - m^2 fails offset, constant per pixel, C = 2 and three more; gate order f, i, c, o in the backward fails every
cell test with a gradient, the recurrence, the aliasing test and the layer.
"""
import copy

import numpy as np
import pytest
import torch

import test_oracle_generator_cells as C
from kccotgan_amd import gan

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32 = torch.float32


@pytest.fixture(scope="module")
def L():
    from kccotgan_amd import _lib
    return _lib


def _place(t, off=0):
    """A device copy of t whose first element lies `off` floats past a 16-byte boundary."""
    buf = torch.full((t.numel() + 8,), float("nan"), device=DEV, dtype=F32)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 * off and v.is_contiguous()
    return v


def _out(shape, off=0):
    return _place(torch.full(tuple(shape), float("nan")), off)


def _call(L, name, *args):
    rc = getattr(L.lib, name)(*args)
    torch.cuda.synchronize()
    assert rc == 0, "%s returned %d: %s" % (name, rc, L.lib.kccot_last_error().decode())


def cell_abi(L, t, dh=True, dc=True, off=0):
    """c, h, dg, dc_prev of one step through the C ABI; dh / dc False = a NULL upstream pointer."""
    B, F4, H, W = t["gx"].shape
    Fn, HW = F4 // 4, H * W
    gx, gh, cp = (_place(t[k], off) for k in ("gx", "gh", "c_prev"))
    c, h, dg, dcp = _out(cp.shape, off), _out(cp.shape, off), _out(gx.shape, off), _out(cp.shape, off)
    _call(L, "kccot_convlstm_cell_fwd_f32", gx.data_ptr(), gh.data_ptr(), cp.data_ptr(), B, Fn, HW, c.data_ptr(), h.data_ptr(), None)
    dH, dC = (_place(t["dh"], off) if dh else None), (_place(t["dc"], off) if dc else None)
    _call(L, "kccot_convlstm_cell_bwd_f32", gx.data_ptr(), gh.data_ptr(), cp.data_ptr(), c.data_ptr(), dH.data_ptr() if dh else None,
          dC.data_ptr() if dc else None, B, Fn, HW, dg.data_ptr(), dcp.data_ptr(), None)
    return {"c": c, "h": h, "dg": dg, "dc_prev": dcp}


def cell_function(t, use_h=True, use_c=True):
    """The same through gan._ConvLSTMCellHIP and autograd: the loss depends on h, on c, or on both."""
    gx, gh, cp = (t[k].to(DEV).requires_grad_(True) for k in ("gx", "gh", "c_prev"))
    c, h = gan._ConvLSTMCellHIP.apply(gx, gh, cp)
    loss = ((h * t["dh"].to(DEV)).sum() if use_h else 0.0) + ((c * t["dc"].to(DEV)).sum() if use_c else 0.0)
    dgx, dgh, dcp = torch.autograd.grad(loss, (gx, gh, cp))
    torch.cuda.synchronize()
    return {"c": c.detach(), "h": h.detach(), "dg": dgx, "dgh": dgh, "dc_prev": dcp}


def check_cell(tag, got, t, dh=True, dc=True):
    ref = C.cell_oracle(t["gx"], t["gh"], t["c_prev"], t["dh"] if dh else None, t["dc"] if dc else None)
    yard = C.cell_yardstick(t, ref, dh, dc)
    worst = max(C.within("%s %s" % (tag, k), got[k], ref[k], yard[k], C.CELL_MARGIN) / max(yard[k], C.FLOOR) for k in C.CELL_OUTPUTS)
    print("WORST cell %s: %.2f x max(yardstick, floor) (margin %d)" % (tag, worst, C.CELL_MARGIN))
    return ref


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ================================================================ ConvLSTM cell
@pytest.mark.parametrize("shape", C.CELL_GENERATOR_SHAPES + C.CELL_EDGE_SHAPES)
def test_cell_against_fp64(L, shape):
    t = C.cell_inputs(shape)
    got = cell_abi(L, t)
    check_cell("%s" % (shape,), got, t)
    fn = cell_function(t)                              # what the generator calls: the same kernels, so the same bits
    assert all(same_bits(fn[k], got[k]) for k in C.CELL_OUTPUTS) and same_bits(fn["dgh"], fn["dg"])


def test_cell_misaligned_buffers_take_the_scalar_kernel_and_give_the_same_values(L):
    B, Fn, H, W = C.CELL_MISALIGNED_SHAPE
    assert (Fn * H * W) % 4 == 0
    t = C.cell_inputs(C.CELL_MISALIGNED_SHAPE, seed=2)
    got = cell_abi(L, t, off=1)
    check_cell("misaligned %s" % (C.CELL_MISALIGNED_SHAPE,), got, t)
    aligned = cell_abi(L, t)
    # the scalar and the vector kernel evaluate the same expressions (contraction off): equal to the last bit
    assert all(same_bits(got[k], aligned[k]) for k in C.CELL_OUTPUTS)


def test_cell_on_and_beside_the_hard_sigmoid_kinks(L):
    t, _ = C.kink_inputs()
    Fn = C.CELL_KINK_SHAPE[1]
    for tag, got in (("kinks abi", cell_abi(L, t)), ("kinks function", cell_function(t))):
        ref = check_cell(tag, got, t)
        dead = torch.from_numpy(ref["mask"] == 0)
        dead[:, 2 * Fn:3 * Fn] = False
        assert int(dead.sum()) > 100
        assert not bool(got["dg"].cpu()[dead].any()), "%s: a gate gradient beyond a kink is not exactly 0" % tag
        live = torch.from_numpy((ref["mask"] != 0) & (np.abs(ref["dg"]) > 1e-6))
        assert bool((got["dg"].cpu()[live] != 0).all()), "%s: a gate gradient on or inside the bounds is 0" % tag


def test_cell_gate_is_the_two_rounding_hard_sigmoid_bit_for_bit(L):
    """c_prev = 0 and a saturated c gate (tanhf(30) = 1: 1 - tanh(30) is 2e-26) leave c = 0 + hsig(g_i) 1: the kernel's input
    gate itself.  It must be clip(fl32(fl32(0.2f g) + 0.5f), 0, 1) exactly -- a fused multiply-add differs in the last bit on a
    good share of these values -- and h = hsig(g_o) tanh(c) to the rule."""
    B, Fn, H, W = shape = (2, 16, 8, 8)
    t = C.cell_inputs(shape, seed=9)
    t["c_prev"] = torch.zeros_like(t["c_prev"])
    t["gx"][:, 2 * Fn:3 * Fn] = 30.0
    t["gh"][:, 2 * Fn:3 * Fn] = 0.0
    t["gx"][:, :Fn] *= 0.4                             # most input gates inside the linear range
    g32 = (t["gx"] + t["gh"]).numpy()
    want = np.clip(C.hard_sigmoid_y32(g32[:, :Fn]), np.float32(0), np.float32(1))
    fused = np.clip((float(np.float32(0.2)) * g32[:, :Fn].astype(np.float64) + 0.5).astype(np.float32), 0, 1)   # one rounding
    print("gate values on which one rounding and two roundings differ: %d of %d" % (int((fused != want).sum()), want.size))
    assert int((fused != want).sum()) > want.size // 20
    got = cell_abi(L, t)
    assert np.array_equal(got["c"].cpu().numpy().view(np.uint32), want.view(np.uint32))
    check_cell("exact gate", got, t)


@pytest.mark.parametrize("dh,dc", [(True, False), (False, True), (True, True), (False, False)])
def test_cell_absent_upstream_gradients(L, dh, dc):
    t = C.cell_inputs(C.CELL_UPSTREAM_SHAPE, seed=3)
    tag = "upstream %s%s" % ("dh" if dh else "", "dc" if dc else "")
    got = cell_abi(L, t, dh, dc)
    if not (dh or dc):
        assert not bool(got["dg"].any()) and not bool(got["dc_prev"].any())
        return
    check_cell(tag + " abi (NULL)", got, t, dh, dc)
    fn = cell_function(t, use_h=dh, use_c=dc)          # autograd hands the Function zeros or None for the unused output
    check_cell(tag + " function", fn, t, dh, dc)
    assert same_bits(fn["dg"], fn["dgh"])


def test_cell_recurrence_over_twelve_steps(L):
    ch = C.chain_inputs()
    ref = C.chain_oracle(ch)
    cpu = C.chain_run(ch, lambda gx, gh, c: gan._cell_torch(gx + gh, c))
    got = C.chain_run(ch, gan._ConvLSTMCellHIP.apply, DEV)
    torch.cuda.synchronize()
    worst = 0.0
    for t in range(C.CELL_CHAIN_T):
        for k, g, r, y in (("h", got["h"][t], ref["h"][t], cpu["h"][t]), ("dgx", got["dgx"][t], ref["dg"][t], cpu["dgx"][t]),
                           ("dgh", got["dgh"][t], ref["dg"][t], cpu["dgh"][t])):
            yard = C.err_of(y, r)
            worst = max(worst, C.within("chain t=%d %s" % (t, k), g, r, yard, C.CELL_MARGIN) / max(yard, C.FLOOR))
    yard = C.err_of(cpu["dc0"], ref["dc0"])
    worst = max(worst, C.within("chain dc0", got["dc0"], ref["dc0"], yard, C.CELL_MARGIN) / max(yard, C.FLOOR))
    print("WORST cell chain: %.2f x max(yardstick, floor) (margin %d)" % (worst, C.CELL_MARGIN))


def test_cell_gradient_returned_twice_accumulates_once_per_leaf(L):
    """_ConvLSTMCellHIP.backward returns ONE tensor for gx and gh.  Two backward passes into leaf .grads must leave twice the
    single-pass gradient in each (x + x is exact), in storage of their own: never three or four times it in a shared one."""
    t = C.cell_inputs((2, 16, 8, 8), seed=4)
    single = cell_function(t)
    ref = C.cell_oracle(t["gx"], t["gh"], t["c_prev"], t["dh"], t["dc"])
    C.within("aliased dg single pass", single["dg"], ref["dg"], C.cell_yardstick(t, ref)["dg"], C.CELL_MARGIN)
    gx, gh = t["gx"].to(DEV).requires_grad_(True), t["gh"].to(DEV).requires_grad_(True)
    cp = t["c_prev"].to(DEV)
    for n in (1, 2):
        c, h = gan._ConvLSTMCellHIP.apply(gx, gh, cp)
        ((h * t["dh"].to(DEV)).sum() + (c * t["dc"].to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        assert torch.equal(gx.grad, n * single["dg"]) and torch.equal(gh.grad, n * single["dg"]), "after %d passes" % n
    assert gx.grad.data_ptr() != gh.grad.data_ptr()
    gx.grad.mul_(0.5)                                   # what gradient clipping does
    assert torch.equal(gx.grad, single["dg"]) and torch.equal(gh.grad, 2 * single["dg"])


# ================================================================ channel LayerNorm
def ln_abi(L, t, eps=C.LN_EPS):
    N, Cn, H, W = t["x"].shape
    HW = H * W
    x, gamma, beta, dy = (_place(t[k]) for k in ("x", "gamma", "beta", "dy"))
    y, mean, rstd, dx = _out(x.shape), _out((N, H, W)), _out((N, H, W)), _out(x.shape)
    nchunk = int(L.lib.kccot_channel_layernorm_chunks(N, Cn, HW))
    parts = _out((nchunk, 2, Cn))
    _call(L, "kccot_channel_layernorm_fwd_f32", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), N, Cn, HW, eps, y.data_ptr(),
          mean.data_ptr(), rstd.data_ptr(), None)
    _call(L, "kccot_channel_layernorm_bwd_f32", dy.data_ptr(), x.data_ptr(), gamma.data_ptr(), mean.data_ptr(), rstd.data_ptr(), N, Cn,
          HW, dx.data_ptr(), parts.data_ptr(), None)
    return {"y": y, "mean": mean, "rstd": rstd, "dx": dx, "partials": parts}


def ln_module(t):
    Cn = t["x"].shape[1]
    ln = gan.ChannelLayerNorm(Cn).to(DEV)
    assert gan._LN_HIP and ln.ln.eps == 1e-3
    with torch.no_grad():
        ln.ln.weight.copy_(t["gamma"])
        ln.ln.bias.copy_(t["beta"])
    x = t["x"].to(DEV).requires_grad_(True)
    y = ln(x)
    dx, dgamma, dbeta = torch.autograd.grad((y * t["dy"].to(DEV)).sum(), [x, ln.ln.weight, ln.ln.bias])
    torch.cuda.synchronize()
    return {"y": y.detach(), "dx": dx, "dgamma": dgamma, "dbeta": dbeta}


@pytest.mark.parametrize("name", sorted(C.LN_CASES))
def test_layernorm_against_fp64(L, name):
    (N, Cn, H, W), kind = C.LN_CASES[name]
    t = C.ln_inputs(name)
    ref = C.ln_oracle(t["x"], t["gamma"], t["beta"], t["dy"])
    yard = C.ln_yardstick(t, ref)
    got = ln_abi(L, t)
    worst = 0.0
    for k in ("mean", "rstd", "y", "dx"):
        worst = max(worst, C.within("%s %s" % (name, k), got[k], ref[k], yard[k], C.LN_MARGIN) / max(yard[k], C.FLOOR))
    # the parameter gradients chunk by chunk: the kernel's ranges are the restated ones, each chunk against the oracle
    # (and the CPU fp32 yardstick) restricted to its samples
    nchunk, _ = C.ln_chunks(N, Cn, H * W)
    assert got["partials"].shape[0] == nchunk
    for k, (n0, n1) in enumerate(C.chunk_ranges(N, nchunk)):
        if nchunk == 1:
            cref, cyard = ref, yard
        else:
            cref = C.ln_oracle(t["x"], t["gamma"], t["beta"], t["dy"], samples=(n0, n1))
            cyard = C.ln_yardstick(t, cref, samples=(n0, n1))
        for j, out in enumerate(("dgamma", "dbeta")):
            worst = max(worst, C.within("%s chunk %d [%d,%d) %s" % (name, k, n0, n1, out), got["partials"][k, j], cref[out], cyard[out],
                                        C.LN_MARGIN) / max(cyard[out], C.FLOOR))
    mod = ln_module(t)                                  # summed over the chunks, as the generator gets them
    assert same_bits(mod["y"], got["y"]) and same_bits(mod["dx"], got["dx"])
    for out in ("dgamma", "dbeta"):
        worst = max(worst, C.within("%s summed %s" % (name, out), mod[out], ref[out], yard[out], C.LN_MARGIN) / max(yard[out], C.FLOOR))
    print("WORST layernorm %s: %.2f x max(yardstick, floor) (margin %d)" % (name, worst, C.LN_MARGIN))
    if Cn == 1:                                         # variance 0: the output is beta and nothing flows back
        assert torch.equal(got["y"].cpu(), t["beta"].view(1, 1, 1, 1).expand(N, Cn, H, W)) and not bool(got["dx"].any())
    if kind == "pixel":
        want = np.float32(1.0) / np.sqrt(np.float32(C.LN_EPS))
        ulps = np.abs(got["rstd"].cpu().numpy().view(np.int32).astype(np.int64) - int(want.view(np.int32)))
        print("%s: rstd within %d ulp of fl32(1 / sqrt(eps)) = %.9g" % (name, int(ulps.max()), float(want)))
        assert int(ulps.max()) <= 2


@pytest.mark.parametrize("name", ["generator 8x64x16x16", "chunks 11x256x4x4", "chunks 9x512x2x2"])
def test_layernorm_zero_upstream_gives_exact_zeros(L, name):
    t = C.ln_inputs(name)
    t["dy"] = torch.zeros_like(t["dy"])
    got = ln_abi(L, t)
    assert not bool(got["dx"].any()) and not bool(got["partials"].any())
    mod = ln_module(t)
    assert not bool(mod["dx"].any()) and not bool(mod["dgamma"].any()) and not bool(mod["dbeta"].any())


def test_layernorm_chunk_count_is_the_restated_one(L):
    C.library_chunks_agree()


# ================================================================ the layer
def test_convlstm_layer_against_fp64():
    """gan.ConvLSTM2D on the fused cell in fp32 against the same module in float64 (which takes the tensor-op path by
    construction), output and every gradient; yardstick: the fp32 tensor-op path on the CPU.  hard_sigmoid decisions may
    legitimately differ between fp32 and float64 hidden states, so the rule is applied to the largest error of each tensor
    against the largest reference value of that tensor; nothing is masked."""
    torch.manual_seed(3)
    layer = gan.ConvLSTM2D(3, 8, 5, 2, (16, 16), bias=True)
    x = torch.randn(2, 6, 3, 16, 16)
    assert gan._CELL_HIP

    def run(m, xin):
        xin = xin.clone().requires_grad_(True)
        with gan.conv_guard():
            y = m(xin)
            gr = torch.autograd.grad((y * y).sum(), [xin] + list(m.parameters()))
        return [y.detach()] + list(gr)

    names = ["y", "dx"] + ["d" + n for n, _ in layer.named_parameters()]
    ref = run(copy.deepcopy(layer).double(), x.double())
    cpu = run(layer, x)
    got = run(copy.deepcopy(layer).to(DEV), x.to(DEV))
    torch.cuda.synchronize()
    worst = 0.0
    for n, g, r, c in zip(names, got, ref, cpu):
        yard = C.err_of(c, r)
        worst = max(worst, C.within("layer %s" % n, g, r, yard, C.LAYER_MARGIN) / max(yard, C.FLOOR))
    print("WORST layer: %.2f x max(yardstick, floor) (margin %d)" % (worst, C.LAYER_MARGIN))
