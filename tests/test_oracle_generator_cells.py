"""The two hand-written kernels on the generator side -- the ConvLSTM cell (csrc/convlstm.hip) and the channel LayerNorm
(csrc/layernorm.hip) -- on float64 oracles alone: the cases, inputs, oracles and yardsticks that
tests/test_gpu_generator_cells_fp64.py runs on the device, and every precondition that module relies on.

* cell_oracle: gate order i, f, c, o.  g32 = gx + gh is ONE fp32 add and y32 = fl32(fl32(0.2f g32) + 0.5f) two fp32
  roundings without a fused multiply-add (NumPy float32) -- the decision arithmetic csrc/convlstm.hip documents, computed
  from the inputs.  Everything after that is float64: gate = clip(y32, 0, 1), gate derivative 0.2 where 0 <= y32 <= 1
  (bounds included) and 0 elsewhere, tanh.  Since the clamp decisions are reproduced exactly no element is ever masked.
  decisions="fp64" takes g and y in float64 instead: only the check against float64 autograd uses it (that one cannot hold
  to 1e-12 across two fp32 roundings).
* ln_oracle: float64 mean, biased variance, rstd, y, dx, dgamma, dbeta (optionally over a range of samples: one chunk of
  the parameter-gradient partition).
* Yardsticks: the largest error of the CPU fp32 tensor-op implementation (gan._cell_torch; nn.LayerNorm on the permuted
  tensor) against the oracle on the same inputs, normalised by max |ref| of that output.  It does not share a line with
  the HIP kernels, so it measures what fp32 costs on these inputs.  The GPU module bounds every comparison by
      |kernel - ref| <= margin max(yardstick, 4 2^-24) max |ref|,      margin 4 (cell, elementwise) or 8 (LayerNorm, sums).
* Chunk arithmetic: ln_chunks / chunk_ranges restate the planner (ln_chunks in csrc/layernorm.hip) and the kernel's own
  per = ceil(N / nchunk) split; the ranges tile [0, N) once, and every "chunk" case has the property it was chosen for.
"""
import numpy as np
import pytest
import torch
import torch.nn as nn

from kccotgan_amd import gan

F32, F64 = torch.float32, torch.float64
U24 = 2.0 ** -24                       # unit roundoff of fp32
FLOOR = 4 * U24                        # the least a yardstick counts for
CELL_MARGIN, LN_MARGIN, LAYER_MARGIN = 4, 8, 8
KINK = 2.5                             # hard_sigmoid = clip(0.2 x + 0.5, 0, 1) bends at x = -2.5 and x = +2.5
LN_EPS = float(np.float32(1e-3))       # Keras' epsilon as the ABI's `float eps` receives it

# ---------------------------------------------------------------- ConvLSTM cell: cases (B, F, H, W)
CELL_GENERATOR_SHAPES = [(2, 32, 32, 32), (2, 64, 16, 16), (2, 128, 8, 8), (2, 256, 4, 4), (2, 8, 64, 64),    # filter_size 8, 64x64
                         (8, 32, 32, 32)]                                                                    # the workload's batch
# F HW not a multiple of 4 (scalar kernel) twice; F HW = 260 (vector kernel, partial last workgroup); one float4 per sample
CELL_EDGE_SHAPES = [(1, 5, 3, 3), (3, 7, 5, 7), (1, 4, 5, 13), (2, 1, 1, 4)]
CELL_MISALIGNED_SHAPE = (2, 8, 4, 4)   # F HW = 128: the vector kernel, unless a base pointer is off its 16 bytes
CELL_KINK_SHAPE = (2, 8, 4, 4)
CELL_UPSTREAM_SHAPE = (3, 7, 5, 7)
CELL_CHAIN_SHAPE, CELL_CHAIN_T = (2, 16, 8, 8), 12


def _gen(*key):
    return torch.Generator().manual_seed(sum((k + 1) * p for k, p in zip(key, (1, 7, 131, 1009, 7919, 104729))))


def cell_inputs(shape, seed=0):
    """fp32 CPU tensors; 4 randn and 2 randn pre-activations as in test_gpu_train_step.py: a good share of gates saturate."""
    B, Fn, H, W = shape
    g = _gen(seed, *shape)
    return {"gx": 4.0 * torch.randn(B, 4 * Fn, H, W, generator=g), "gh": 2.0 * torch.randn(B, 4 * Fn, H, W, generator=g),
            "c_prev": torch.randn(B, Fn, H, W, generator=g), "dh": torch.randn(B, Fn, H, W, generator=g),
            "dc": torch.randn(B, Fn, H, W, generator=g)}


def kink_values():
    """fp32 pre-activation sums on and beside both kinks, and the far ends: +-2.5, their fp32 neighbours on both sides,
    +-2.5 (1 +- 2^-20), 0 (as 1 + -1), +-1e30, +0.0, -0.0."""
    f = np.float32
    out = []
    for s in (1.0, -1.0):
        k = f(KINK * s)
        out += [k, np.nextafter(k, f(np.inf)), np.nextafter(k, f(-np.inf)), f(KINK * s * (1 + 2.0 ** -20)), f(KINK * s * (1 - 2.0 ** -20))]
    out += [f(0.0), f(1e30), f(-1e30), f(0.0), f(-0.0)]
    return np.array(out, np.float32)


def split_exact(v, k):
    """(a, b) fp32 with fl32(a + b) == v, sign of zero included.  a = +-1 where v - a is an fp32 number, else a = b = v / 2
    (exact: a power of two); entry 14 of kink_values (-0.0) and entry 13 (+0.0) are halved, entry 10 (0) is 1 + -1."""
    v = np.float32(v)
    if k not in (13, 14) and abs(float(v)) < 1e6:
        a = np.float32(-1.0 if np.signbit(v) else 1.0)
        b = np.float32(float(v) - float(a))
        if float(a) + float(b) == float(v):
            return a, b
    return np.float32(v / np.float32(2)), np.float32(v / np.float32(2))


def kink_inputs():
    """CELL_KINK_SHAPE: the i, f and o sums cycle through kink_values() (each gate at its own stride, so the combinations
    vary), the c gate, c_prev and both upstream gradients are random.  Returns (inputs, value index [B, 3, F, H, W])."""
    B, Fn, H, W = CELL_KINK_SHAPE
    vals = kink_values()
    nv, n = len(vals), B * Fn * H * W
    t = cell_inputs(CELL_KINK_SHAPE, seed=5)
    gx, gh = t["gx"].numpy().copy(), t["gh"].numpy().copy()
    k = np.arange(n).reshape(B, Fn, H, W)
    idx = np.stack([k % nv, (2 * k + 3) % nv, (4 * k + 7) % nv], axis=1)
    for q, gate in enumerate((0, 1, 3)):
        for pos in np.ndindex(B, Fn, H, W):
            a, b = split_exact(vals[idx[(pos[0], q) + pos[1:]]], int(idx[(pos[0], q) + pos[1:]]))
            gx[pos[0], gate * Fn + pos[1], pos[2], pos[3]] = a
            gh[pos[0], gate * Fn + pos[1], pos[2], pos[3]] = b
    t["gx"], t["gh"] = torch.from_numpy(gx), torch.from_numpy(gh)
    return t, idx


def _np(t, dtype):
    return None if t is None else np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).astype(dtype, copy=False)


def hard_sigmoid_y32(g32):
    """fl32(fl32(0.2f g) + 0.5f): NumPy rounds the product and the sum separately."""
    assert g32.dtype == np.float32
    y = np.float32(0.2) * g32
    y = y + np.float32(0.5)
    assert y.dtype == np.float32
    return y


def cell_oracle(gx, gh, c_prev, dh=None, dc=None, decisions="fp32"):
    """float64 c, h, dg [B,4F,H,W], dc_prev of one cell step, on the fp32 values of gx, gh (c_prev, dh, dc: any precision;
    dh or dc None = absent).  Also y (the value the clamp decides on) and mask (the gate derivative)."""
    cp = _np(c_prev, np.float64)
    Fn = cp.shape[1]
    if decisions == "fp32":
        g32 = _np(gx, np.float32) + _np(gh, np.float32)
        assert g32.dtype == np.float32
        y, g = hard_sigmoid_y32(g32).astype(np.float64), g32.astype(np.float64)
    else:
        g = _np(gx, np.float64) + _np(gh, np.float64)
        y = 0.2 * g + 0.5
    gate = np.clip(y, 0.0, 1.0)
    mask = np.where((y >= 0.0) & (y <= 1.0), 0.2, 0.0)
    i, f, o = gate[:, :Fn], gate[:, Fn:2 * Fn], gate[:, 3 * Fn:]
    mi, mf, mo = mask[:, :Fn], mask[:, Fn:2 * Fn], mask[:, 3 * Fn:]
    cc = np.tanh(g[:, 2 * Fn:3 * Fn])
    c = f * cp + i * cc
    tc = np.tanh(c)
    h = o * tc
    dH = np.zeros_like(c) if dh is None else _np(dh, np.float64)
    dC = np.zeros_like(c) if dc is None else _np(dc, np.float64)
    dcj = dC + dH * o * (1.0 - tc * tc)
    dg = np.concatenate([dcj * cc * mi, dcj * cp * mf, dcj * i * (1.0 - cc * cc), dH * tc * mo], axis=1)
    return {"c": c, "h": h, "dg": dg, "dc_prev": dcj * f, "y": y, "mask": mask}


CELL_OUTPUTS = ("c", "h", "dg", "dc_prev")


def cell_tensor_ops(gx, gh, c_prev, dh=None, dc=None, dtype=F32):
    """gan._cell_torch on CPU tensors in `dtype`, gradients by autograd: c, h, dgx, dgh, dc_prev (NumPy float64)."""
    a = [t.detach().cpu().to(dtype).requires_grad_(True) for t in (gx, gh, c_prev)]
    c, h = gan._cell_torch(a[0] + a[1], a[2])
    out = {"c": _np(c, np.float64), "h": _np(h, np.float64)}
    loss = 0.0
    if dh is not None:
        loss = loss + (h * dh.detach().cpu().to(dtype)).sum()
    if dc is not None:
        loss = loss + (c * dc.detach().cpu().to(dtype)).sum()
    if dh is not None or dc is not None:
        grads = torch.autograd.grad(loss, a)
        out.update(dg=_np(grads[0], np.float64), dgh=_np(grads[1], np.float64), dc_prev=_np(grads[2], np.float64))
    return out


def err_of(got, ref):
    """max |got - ref| / max |ref| (an all-zero reference: the absolute error)."""
    got, ref = _np(got, np.float64), _np(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite values"
    norm = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (norm if norm > 0 else 1.0)


def cell_yardstick(t, ref=None, dh=True, dc=True):
    """{output: error of the CPU fp32 tensor-op cell against the oracle} on the inputs t (cell_inputs / kink_inputs)."""
    dh, dc = (t["dh"] if dh else None), (t["dc"] if dc else None)
    ref = ref or cell_oracle(t["gx"], t["gh"], t["c_prev"], dh, dc)
    got = cell_tensor_ops(t["gx"], t["gh"], t["c_prev"], dh, dc)
    return {k: err_of(got[k], ref[k]) for k in CELL_OUTPUTS if k in got}


def within(tag, got, ref, yard, margin):
    """The tolerance rule of the GPU module; prints the figures, returns the error.  Every element is compared.  A reference
    that is zero everywhere leaves the rule no room: the values must be exactly 0."""
    err, norm = err_of(got, ref), float(np.abs(_np(ref, np.float64)).max())
    if norm == 0:
        print("%s: reference exactly 0, largest |value| %.3e" % (tag, err))
        assert err == 0, "%s: the reference is exactly 0, got up to %.3e" % (tag, err)
        return 0.0
    tol = margin * max(yard, FLOOR)
    print("%s: err %.3e  yardstick %.3e  bound %.3e (margin %d)  max|ref| %.3e  -> %.2f of the bound"
          % (tag, err, yard, tol, margin, norm, err / tol))
    assert err <= tol, "%s: %.3e exceeds %d x max(%.3e, 4 x 2^-24) = %.3e (of max |ref| = %.3e)" % (tag, err, margin, yard, tol, norm)
    return err


# ---------------------------------------------------------------- the recurrence
def chain_inputs():
    B, Fn, H, W = CELL_CHAIN_SHAPE
    g = _gen(12, *CELL_CHAIN_SHAPE)
    r = lambda s, *shape: s * torch.randn(*shape, generator=g)
    return {"gx": [r(4.0, B, 4 * Fn, H, W) for _ in range(CELL_CHAIN_T)], "gh": [r(2.0, B, 4 * Fn, H, W) for _ in range(CELL_CHAIN_T)],
            "w": [r(1.0, B, Fn, H, W) for _ in range(CELL_CHAIN_T)], "c0": r(1.0, B, Fn, H, W)}


def chain_oracle(ch, decisions="fp32"):
    """loss = sum_t <h_t, w_t>, c threaded through T steps (in float64): h_t, and the gradients w.r.t. every gx_t (== gh_t)
    and c_0, by running cell_oracle backwards over the chain; dc is absent at the last step."""
    T = len(ch["gx"])
    cs, hs = [_np(ch["c0"], np.float64)], []
    for t in range(T):
        o = cell_oracle(ch["gx"][t], ch["gh"][t], cs[-1], decisions=decisions)
        cs.append(o["c"])
        hs.append(o["h"])
    dgs, dc = [None] * T, None
    for t in reversed(range(T)):
        o = cell_oracle(ch["gx"][t], ch["gh"][t], cs[t], ch["w"][t], dc, decisions=decisions)
        dgs[t], dc = o["dg"], o["dc_prev"]
    return {"h": hs, "dg": dgs, "dc0": dc}


def chain_run(ch, cell, device="cpu"):
    """The same chain through `cell(gx, gh, c) -> c, h` on fp32 leaves; returns h_t, gx_t.grad, gh_t.grad, c0.grad."""
    leaf = lambda t: t.detach().clone().to(device).requires_grad_(True)      # never the caller's tensor itself
    gx, gh, c0 = [leaf(t) for t in ch["gx"]], [leaf(t) for t in ch["gh"]], leaf(ch["c0"])
    c, hs, loss = c0, [], 0.0
    for t in range(len(gx)):
        c, h = cell(gx[t], gh[t], c)
        hs.append(h)
        loss = loss + (h * ch["w"][t].to(device)).sum()
    loss.backward()
    return {"h": [h.detach() for h in hs], "dgx": [t.grad for t in gx], "dgh": [t.grad for t in gh], "dc0": c0.grad}


# ---------------------------------------------------------------- channel LayerNorm: cases name -> ((N, C, H, W), input kind)
LN_GENERATOR_SHAPES = [(8, 32, 32, 32), (8, 64, 16, 16), (8, 128, 8, 8), (8, 256, 4, 4), (8, 16, 64, 64), (8, 8, 64, 64)]
# shape -> (nchunk, planner's per, kernel's per, samples in the last chunk): the property each was chosen for
LN_CHUNK_CASES = {(11, 256, 4, 4): (6, 2, 2, 1),          # 2 samples per chunk, ragged last chunk
                  (9, 512, 2, 2): (2, 8, 5, 4),           # the planner's per differs from the kernel's
                  (40, 16, 4, 4): (40, 1, 1, 1),          # one sample per chunk
                  (2, 3, 257, 257): (2, 1, 1, 1),         # H W > 65536: per clamps to 1
                  (1, 3, 33, 17): (1, 116, 1, 1)}         # a single chunk; H W neither a multiple of 256 nor of 4
LN_CASES = {}
for _s in LN_GENERATOR_SHAPES:
    LN_CASES["generator %dx%dx%dx%d" % _s] = (_s, "tanh")
for _s in LN_CHUNK_CASES:
    LN_CASES["chunks %dx%dx%dx%d" % _s] = (_s, "randn")
LN_CASES.update({"C=1": ((4, 1, 8, 8), "randn"), "C=2": ((4, 2, 8, 8), "randn"), "offset": ((4, 64, 8, 8), "offset"),
                 "tiny": ((4, 64, 8, 8), "tiny"), "constant per pixel": ((4, 64, 8, 8), "pixel")})
LN_CHUNK_TARGET = 64 * 1024            # LN_CHUNK_SAMPLES_TARGET of csrc/layernorm.hip


def ln_inputs(name):
    """fp32 CPU tensors x, gamma = |randn| + 0.5, beta = randn, dy = randn."""
    shape, kind = LN_CASES[name]
    N, C, H, W = shape
    g = _gen(sorted(LN_CASES).index(name), *shape)
    r = torch.randn(shape, generator=g)
    if kind == "tanh":
        x = torch.tanh(1.5 * r)                                        # what the generator's layers feed it
    elif kind == "randn":
        x = 2.0 * r + 0.7                                              # test_gpu_train_step.py
    elif kind == "offset":
        x = 8.0 + 0.5 * r                                              # a common offset sixteen times the spread
    elif kind == "tiny":
        x = 1e-4 * r                                                   # eps dominates
    else:
        x = r[:, :1].expand(shape).contiguous()                        # the same value in every channel of a pixel
    return {"x": x, "gamma": torch.randn(C, generator=g).abs() + 0.5, "beta": torch.randn(C, generator=g),
            "dy": torch.randn(shape, generator=g)}


def ln_oracle(x, gamma, beta, dy=None, eps=LN_EPS, samples=None):
    """float64 mean, rstd [N,H,W], y and (with dy) dx [N,C,H,W], dgamma, dbeta [C] on the given values; samples = (n0, n1)
    restricts everything to that range of the batch (one chunk of the parameter gradients)."""
    sl = slice(*samples) if samples is not None else slice(None)
    x, gm, bt = _np(x, np.float64)[sl], _np(gamma, np.float64)[None, :, None, None], _np(beta, np.float64)[None, :, None, None]
    mean = x.mean(axis=1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    xh = (x - mean) * rstd
    out = {"mean": mean[:, 0], "rstd": rstd[:, 0], "y": xh * gm + bt}
    if dy is not None:
        dy = _np(dy, np.float64)[sl]
        dg = dy * gm
        out["dx"] = rstd * (dg - dg.mean(axis=1, keepdims=True) - xh * (dg * xh).mean(axis=1, keepdims=True))
        out["dgamma"], out["dbeta"] = (dy * xh).sum(axis=(0, 2, 3)), dy.sum(axis=(0, 2, 3))
    return out


LN_OUTPUTS = ("mean", "rstd", "y", "dx", "dgamma", "dbeta")


def ln_tensor_ops(x, gamma, beta, dy=None, eps=LN_EPS, samples=None, dtype=F32):
    """nn.LayerNorm on the permuted CPU tensor in `dtype`, gradients by autograd; mean and rstd are those of
    torch.native_layer_norm, the function nn.LayerNorm ends in.  NumPy float64, NCHW."""
    sl = slice(*samples) if samples is not None else slice(None)
    C = x.shape[1]
    ln = nn.LayerNorm(C, eps=eps).to(dtype)
    with torch.no_grad():
        ln.weight.copy_(gamma.detach().cpu().to(dtype))
        ln.bias.copy_(beta.detach().cpu().to(dtype))
    xs = x.detach().cpu().to(dtype)[sl].clone().requires_grad_(True)
    y = ln(xs.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)
    _, mean, rstd = torch.native_layer_norm(xs.detach().permute(0, 2, 3, 1).contiguous(), (C,), ln.weight.detach(), ln.bias.detach(), eps)
    out = {"y": _np(y, np.float64), "mean": _np(mean[..., 0], np.float64), "rstd": _np(rstd[..., 0], np.float64)}
    if dy is not None:
        gr = torch.autograd.grad((y * dy.detach().cpu().to(dtype)[sl]).sum(), [xs, ln.weight, ln.bias])
        out.update(dx=_np(gr[0], np.float64), dgamma=_np(gr[1], np.float64), dbeta=_np(gr[2], np.float64))
    return out


def ln_yardstick(t, ref=None, samples=None):
    """{output: error of the CPU fp32 nn.LayerNorm against the oracle} on the inputs t (ln_inputs)."""
    ref = ref or ln_oracle(t["x"], t["gamma"], t["beta"], t["dy"], samples=samples)
    got = ln_tensor_ops(t["x"], t["gamma"], t["beta"], t["dy"], samples=samples)
    return {k: err_of(got[k], ref[k]) for k in LN_OUTPUTS}


def ln_chunks(N, C, HW):
    """(nchunk, the planner's samples per chunk): ln_chunks of csrc/layernorm.hip, restated."""
    per = max(LN_CHUNK_TARGET // HW, 1)
    ch = (N + per - 1) // per
    while ch * C < 1024 and ch < N:
        per = (per + 1) // 2
        ch = (N + per - 1) // per
    return ch, per


def chunk_ranges(N, nchunk):
    """[n0, n1) of every chunk as chan_ln_bwd_params takes them: per = ceil(N / nchunk), NOT the planner's per."""
    per = (N + nchunk - 1) // nchunk
    return [(min(k * per, N), min(k * per + per, N)) for k in range(nchunk)]


# ================================================================ CPU checks
def _push_off_the_kinks(t, least=1e-3):
    """Move every i, f, o sum that lies within `least` of a kink away from it (by 0.01, into gx)."""
    Fn = t["c_prev"].shape[1]
    gx = t["gx"].clone()
    near = ((gx + t["gh"]).abs() - KINK).abs() < 2 * least
    near[:, 2 * Fn:3 * Fn] = False
    gx[near] += 0.01 * torch.sign(gx[near] + t["gh"][near])
    t = dict(t, gx=gx)
    g = (t["gx"].double() + t["gh"].double())
    g = torch.cat([g[:, :2 * Fn], g[:, 3 * Fn:]], 1)
    assert float(((g.abs() - KINK).abs()).min()) >= least
    return t


@pytest.mark.parametrize("shape", [(2, 16, 8, 8), (3, 7, 5, 7), (2, 8, 64, 64)])
@pytest.mark.parametrize("dh,dc", [(True, True), (True, False), (False, True)])
def test_cell_oracle_is_the_float64_autograd_of_the_tensor_op_cell(shape, dh, dc):
    t = _push_off_the_kinks(cell_inputs(shape, seed=1))
    up = (t["dh"] if dh else None), (t["dc"] if dc else None)
    ref = cell_oracle(t["gx"], t["gh"], t["c_prev"], *up, decisions="fp64")
    got = cell_tensor_ops(t["gx"], t["gh"], t["c_prev"], *up, dtype=F64)
    assert np.array_equal(got["dg"], got["dgh"])
    for k in CELL_OUTPUTS:
        assert err_of(ref[k], got[k]) <= 1e-12, k
    # the fp32 decision arithmetic moves nothing but roundings of g and y this far from a kink: one rounding of g
    # (2^-24 |g|, |g| <= 32 here, through a slope of at most 1 into c and h) and two of y
    own = cell_oracle(t["gx"], t["gh"], t["c_prev"], *up)
    assert np.array_equal(own["mask"], ref["mask"])
    for k in ("c", "h"):
        assert float(np.abs(own[k] - ref[k]).max()) <= 40 * U24, k


def test_kink_inputs_sum_exactly_to_the_kink_values():
    t, idx = kink_inputs()
    vals = kink_values()
    B, Fn, H, W = CELL_KINK_SHAPE
    g32 = (t["gx"] + t["gh"]).numpy()
    exact = t["gx"].double().numpy() + t["gh"].double().numpy()
    for q, gate in enumerate((0, 1, 3)):
        assert np.array_equal(exact[:, gate * Fn:(gate + 1) * Fn], g32[:, gate * Fn:(gate + 1) * Fn].astype(np.float64)), "the fp32 sum is not exact"
        got, want = g32[:, gate * Fn:(gate + 1) * Fn], vals[idx[:, q]]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "gate %d (sign of zero included)" % gate
        assert set(idx[:, q].reshape(-1).tolist()) == set(range(len(vals)))
    # the list is what it says: the kinks, both neighbours of each, 2.5 (1 +- 2^-20), zeros of both signs, the far ends
    assert len(vals) == 15 and vals[0] == 2.5 and vals[5] == -2.5
    for k in (0, 5):
        assert vals[k + 1] > vals[k] > vals[k + 2] and float(vals[k + 1]) - float(vals[k + 2]) == 2.0 ** -21
        assert abs(abs(float(vals[k + 3])) - 2.5 * (1 + 2.0 ** -20)) <= 2.0 ** -23 and abs(abs(float(vals[k + 4])) - 2.5 * (1 - 2.0 ** -20)) <= 2.0 ** -23
    assert np.signbit(vals[14]) and not np.signbit(vals[13]) and vals[11] == np.float32(1e30) and vals[12] == np.float32(-1e30)
    # every decision occurs, on each of the three gates: below, on the lower bound, inside, on the upper bound, above
    y = cell_oracle(t["gx"], t["gh"], t["c_prev"])["y"]
    for gate in (0, 1, 3):
        yg = y[:, gate * Fn:(gate + 1) * Fn]
        assert (yg < 0).any() and (yg == 0).any() and ((yg > 0) & (yg < 1)).any() and (yg == 1).any() and (yg > 1).any()


def _beside_the_kinks():
    """fp32 values: every number within 64 ulp of either kink, the kink values, and 20000 random ones across the range."""
    out = [kink_values()]
    for s in (1.0, -1.0):
        v = np.float32(KINK * s)
        out.append((v.view(np.uint32) + np.arange(-64, 65)).astype(np.uint32).view(np.float32))
    out.append((4.0 * torch.randn(20000, generator=_gen(3))).numpy())
    return np.concatenate(out)


def test_oracle_clamp_decisions_are_those_of_the_fp32_hard_sigmoid():
    """y32 < 0, y32 > 1 and in between, against gan.hard_sigmoid on fp32 CPU tensors: the forward value is clip(y32, 0, 1)
    bit for bit, and torch.clamp's gradient is 0.2 exactly where 0 <= y32 <= 1 (bounds included) and 0 elsewhere.  Value and
    gradient together fix the three-way decision."""
    t, _ = kink_inputs()
    for g32 in (_beside_the_kinks(), (t["gx"] + t["gh"]).numpy().reshape(-1)):
        y32 = hard_sigmoid_y32(g32)
        x = torch.from_numpy(g32.copy()).requires_grad_(True)
        hs = gan.hard_sigmoid(x)
        grad, = torch.autograd.grad(hs.sum(), x)
        assert hs.dtype == F32
        assert np.array_equal(hs.detach().numpy().view(np.uint32), np.clip(y32, np.float32(0), np.float32(1)).view(np.uint32))
        inside = (y32 >= 0) & (y32 <= 1)
        assert np.array_equal(grad.numpy(), np.where(inside, np.float32(0.2), np.float32(0)))
        below, above = (grad.numpy() == 0) & (hs.detach().numpy() == 0), (grad.numpy() == 0) & (hs.detach().numpy() == 1)
        assert np.array_equal(below, y32 < 0) and np.array_equal(above, y32 > 1)
    # on the kinks themselves the bounds are met exactly and the gradient passes: fl32(0.2f 2.5f) = 0.5
    y = hard_sigmoid_y32(np.array([2.5, -2.5], np.float32))
    assert y[0] == 1.0 and y[1] == 0.0


def test_oracle_mask_on_the_kink_case_is_the_fp32_autograd_pattern():
    t, _ = kink_inputs()
    ref = cell_oracle(t["gx"], t["gh"], t["c_prev"], t["dh"], t["dc"])
    got = cell_tensor_ops(t["gx"], t["gh"], t["c_prev"], t["dh"], t["dc"])
    Fn = CELL_KINK_SHAPE[1]
    for gate in (0, 1, 3):
        sl = slice(gate * Fn, (gate + 1) * Fn)
        dead = ref["mask"][:, sl] == 0
        assert dead.any() and not dead.all()
        assert not got["dg"][:, sl][dead].any() and not ref["dg"][:, sl][dead].any()
        live = ~dead & (np.abs(ref["dg"][:, sl]) > 1e-6)
        assert live.any() and (got["dg"][:, sl][live] != 0).all()
    yard = cell_yardstick(t, ref)
    assert all(v <= 8 * U24 for v in yard.values()), yard          # the tensor-op cell takes every decision as the oracle does


def test_chain_oracle_is_the_float64_autograd_of_the_chain():
    """Off the kinks (every step's i, f, o sums at least 1e-3 away), with g and y taken in float64 as autograd takes them."""
    ch = chain_inputs()
    for t in range(CELL_CHAIN_T):
        ch["gx"][t] = _push_off_the_kinks({"gx": ch["gx"][t], "gh": ch["gh"][t], "c_prev": ch["c0"]})["gx"]
    ref = chain_oracle(ch, decisions="fp64")
    cell = lambda gx, gh, c: gan._cell_torch(gx + gh, c)
    got = chain_run({k: ([v.double() for v in vs] if isinstance(vs, list) else vs.double()) for k, vs in ch.items()}, cell)
    for t in range(CELL_CHAIN_T):
        assert err_of(ref["h"][t], got["h"][t]) <= 1e-12 and err_of(ref["dg"][t], got["dgx"][t]) <= 1e-12
        assert np.array_equal(_np(got["dgx"][t], np.float64), _np(got["dgh"][t], np.float64))
    assert err_of(ref["dc0"], got["dc0"]) <= 1e-12
    assert float(np.abs(ref["dc0"]).max()) > 1e-3 and float(np.abs(ref["dg"][0]).max()) > 1e-3      # the gradient reaches step 0


@pytest.mark.parametrize("name", sorted(LN_CASES))
def test_ln_oracle_is_the_float64_autograd_of_nn_layernorm(name):
    samples = None
    t = ln_inputs(name)
    ref = ln_oracle(t["x"], t["gamma"], t["beta"], t["dy"], samples=samples)
    got = ln_tensor_ops(t["x"], t["gamma"], t["beta"], t["dy"], samples=samples, dtype=F64)
    for k in LN_OUTPUTS:
        norm = float(np.abs(ref[k]).max())       # an exactly zero reference (variance 0): autograd's own rounding, absolutely
        assert float(np.abs(ref[k] - got[k]).max()) <= 1e-12 * (norm if norm > 0 else 1.0), k


def test_ln_oracle_exact_cases():
    t = ln_inputs("C=1")
    ref = ln_oracle(t["x"], t["gamma"], t["beta"], t["dy"])
    assert np.array_equal(ref["y"], np.broadcast_to(t["beta"].double().numpy()[None, :, None, None], ref["y"].shape)) and not ref["dx"].any()
    t = ln_inputs("constant per pixel")
    assert bool((t["x"] == t["x"][:, :1]).all())
    ref = ln_oracle(t["x"], t["gamma"], t["beta"], t["dy"])
    assert np.array_equal(ref["y"], np.broadcast_to(t["beta"].double().numpy()[None, :, None, None], ref["y"].shape))
    assert np.array_equal(ref["rstd"], np.full(ref["rstd"].shape, 1.0 / np.sqrt(LN_EPS)))
    t = ln_inputs("offset")
    assert abs(float(t["x"].mean()) - 8.0) < 0.05 and abs(float(t["x"].std()) - 0.5) < 0.02


@pytest.mark.parametrize("name", sorted(LN_CASES))
def test_chunk_ranges_tile_the_batch(name):
    (N, C, H, W), _ = LN_CASES[name]
    nchunk, per = ln_chunks(N, C, H * W)
    assert 1 <= nchunk <= N and per >= 1 and (N + per - 1) // per == nchunk
    ranges = chunk_ranges(N, nchunk)
    assert len(ranges) == nchunk
    assert [n for n0, n1 in ranges for n in range(n0, n1)] == list(range(N)), "the chunks do not tile [0, N) exactly once"


@pytest.mark.parametrize("shape", sorted(LN_CHUNK_CASES))
def test_chunk_cases_have_the_property_they_were_chosen_for(shape):
    N, C, H, W = shape
    nchunk, per = ln_chunks(N, C, H * W)
    ranges = chunk_ranges(N, nchunk)
    kernel_per = ranges[0][1] - ranges[0][0]
    assert (nchunk, per, kernel_per, ranges[-1][1] - ranges[-1][0]) == LN_CHUNK_CASES[shape]
    if shape == (11, 256, 4, 4):
        assert [b - a for a, b in ranges] == [2, 2, 2, 2, 2, 1]
    if shape == (9, 512, 2, 2):
        assert per != kernel_per and ranges == [(0, 5), (5, 9)]
    if shape == (2, 3, 257, 257):
        assert H * W > LN_CHUNK_TARGET and LN_CHUNK_TARGET // (H * W) == 0
    if shape == (1, 3, 33, 17):
        assert (H * W) % 256 and (H * W) % 4


def library_chunks_agree():
    """kccot_channel_layernorm_chunks (host code: no GPU involved) against the restatement, for every LayerNorm case."""
    from kccotgan_amd import _lib
    for name, ((N, C, H, W), _) in sorted(LN_CASES.items()):
        assert int(_lib.lib.kccot_channel_layernorm_chunks(N, C, H * W)) == ln_chunks(N, C, H * W)[0], name


def test_chunk_count_is_the_library_s():
    try:
        from kccotgan_amd import _lib  # noqa: F401
    except (ImportError, OSError) as e:          # the GPU module makes the comparison where the library cannot load here
        pytest.skip("libkccot.so does not load on this machine: %s" % e)
    library_chunks_agree()


@pytest.mark.parametrize("name", ["generator 8x64x16x16", "chunks 11x256x4x4", "offset", "tiny", "C=2"])
def test_ln_yardstick_is_fp32_sized(name):
    """The CPU fp32 nn.LayerNorm is an fp32 computation of these inputs: its error is a small multiple of 2^-24 of max |ref|,
    not orders above rounding (64 x 2^-24 leaves room for the offset case, whose condition number is 16), so the GPU
    module's bound means what it says.  (The two variance-0 cases have exactly zero references: see `within`.)"""
    t = ln_inputs(name)
    yard = ln_yardstick(t)
    print(name, {k: "%.2e" % v for k, v in yard.items()})
    assert all(v <= 64 * U24 for v in yard.values()), yard


@pytest.mark.parametrize("shape", [(2, 64, 16, 16), (3, 7, 5, 7)])
def test_cell_yardstick_is_fp32_sized(shape):
    yard = cell_yardstick(cell_inputs(shape))
    print(shape, {k: "%.2e" % v for k, v in yard.items()})
    assert all(0 < v <= 16 * U24 for v in yard.values()), yard
