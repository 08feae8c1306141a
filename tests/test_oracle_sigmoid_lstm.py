"""CPU tier of the sigmoid-LSTM kernels (csrc/sigmoid_lstm.hip, include/kccot_models.h): a float64 NumPy oracle of the
forward recurrence and of full back-propagation through time, proven here against float64 autograd of gan._SigmoidLSTM's own
loop; the yardstick of the GPU module (tests/test_gpu_sigmoid_lstm.py: the error of the CPU fp32 tensor-op loop against the
oracle on the same inputs); the header as strict C99; the exported symbols against _lib.MODEL_SIGNATURES; and the argument
checks that need no GPU.  Cases and inputs are shared with the GPU module, computed once."""
import ctypes
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from kccotgan_amd import gan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = torch.float32, torch.float64
U24 = 2.0 ** -24
FLOOR = 4 * U24                        # the least a yardstick counts for
MARGIN = 8                             # tests/test_gpu_generator_cells_fp64.py: kernels that sum in another order than the yardstick

# (B, T, U).  The trainer's own shape at BASELINE configs[1]; B = 1, 3, 67: one sample, a partial lane group, several waves and
# a partial one (8 samples per wave at U = 8); T = 1, 2: no carry at all, one carry; U = 1, 3, 16, 64 and every lane-group width
# in between (2; 5: partial group of 8; 17 and 33: the LDS kernels with a partial group).
TRAINER = (64, 30, 8)
EDGES = [(1, 30, 8), (3, 5, 8), (67, 7, 8), (3, 1, 8), (3, 2, 8), (67, 3, 1), (5, 6, 3), (5, 6, 16), (3, 6, 64), (67, 2, 3), (3, 4, 2),
         (9, 4, 5), (3, 4, 17), (2, 4, 33), (1, 1, 1)]
CASES = [TRAINER] + EDGES
SATURATED = (8, 12, 8)                 # gx scaled by 20
MODULE_CASES = [(64, 30, 32, 8), (3, 5, 7, 3), (67, 2, 5, 16), (2, 1, 4, 64)]      # (B, T, F, U) through gan._SigmoidLSTM


def _gen(*key):
    return torch.Generator().manual_seed(sum((k + 1) * p for k, p in zip(key, (1, 7, 131, 1009, 7919, 104729))))


@functools.lru_cache(maxsize=None)
def inputs(shape, scale=1.0, seed=0):
    """fp32 CPU tensors: gx ~ N(0, scale^2) [B,T,4U], wh ~ U(-2/sqrt(U), 2/sqrt(U)) [4U,U], upstream dh ~ N(0,1) [B,T,U]."""
    B, T, U = shape
    g = _gen(seed, B, T, U)
    return {"gx": scale * torch.randn(B, T, 4 * U, generator=g), "wh": (torch.rand(4 * U, U, generator=g) * 2 - 1) * (2.0 / U ** 0.5),
            "dh": torch.randn(B, T, U, generator=g)}


def _sig(x):
    """Logistic sigmoid in float64 without overflow."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _np64(t):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t).astype(np.float64)


def oracle(gx, wh, dh=None):
    """float64 h_seq, c_seq [B,T,U] and, with an upstream dh [B,T,U], dgx [B,T,4U] and dwh [4U,U] of the layer: gate order
    i, f, c, o; h_{-1} = c_{-1} = 0; g = gx_t + wh h_{t-1}; c = s(g_f) c + s(g_i) s(g_c); h = s(g_o) s(c)."""
    gx, wh = _np64(gx), _np64(wh)
    B, T, U4 = gx.shape
    U = U4 // 4
    h, c = np.zeros((B, U)), np.zeros((B, U))
    hs, cs, gates = np.zeros((B, T, U)), np.zeros((B, T, U)), np.zeros((B, T, 4, U))
    for t in range(T):
        g = (gx[:, t] + h @ wh.T).reshape(B, 4, U)
        a = _sig(g)
        c = a[:, 1] * c + a[:, 0] * a[:, 2]
        h = a[:, 3] * _sig(c)
        hs[:, t], cs[:, t], gates[:, t] = h, c, a
    out = {"h_seq": hs, "c_seq": cs}
    if dh is None:
        return out
    dh = _np64(dh)
    dgx, dwh = np.zeros((B, T, 4, U)), np.zeros((4 * U, U))
    dh_carry, dc_carry = np.zeros((B, U)), np.zeros((B, U))
    for t in range(T - 1, -1, -1):
        i, f, cc, o = (gates[:, t, q] for q in range(4))
        sc = _sig(cs[:, t])
        c_prev = cs[:, t - 1] if t > 0 else np.zeros((B, U))
        h_prev = hs[:, t - 1] if t > 0 else np.zeros((B, U))
        dht = dh[:, t] + dh_carry
        dct = dc_carry + dht * o * sc * (1 - sc)
        dgx[:, t, 0] = dct * cc * i * (1 - i)
        dgx[:, t, 1] = dct * c_prev * f * (1 - f)
        dgx[:, t, 2] = dct * i * cc * (1 - cc)
        dgx[:, t, 3] = dht * sc * o * (1 - o)
        dg = dgx[:, t].reshape(B, 4 * U)
        dwh += dg.T @ h_prev
        dh_carry = dg @ wh
        dc_carry = dct * f
    out.update(dgx=dgx.reshape(B, T, 4 * U), dwh=dwh)
    return out


def loop(gx, wh, dh=None, dtype=F32):
    """The tensor-op loop of gan._SigmoidLSTM.forward on (gx, wh) -- the same expressions, with the cell state kept -- on the
    CPU in `dtype`, gradients by autograd; NumPy float64."""
    gx = gx.detach().cpu().to(dtype).requires_grad_(True)
    wh = wh.detach().cpu().to(dtype).requires_grad_(True)
    B, T, U = gx.shape[0], gx.shape[1], wh.shape[1]
    h = gx.new_zeros(B, U)
    c = torch.zeros_like(h)
    hs, cs = [], []
    for t in range(T):
        gi, gf, gc, go = torch.chunk(gx[:, t] + torch.nn.functional.linear(h, wh), 4, dim=1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.sigmoid(gc)
        h = torch.sigmoid(go) * torch.sigmoid(c)
        hs.append(h)
        cs.append(c)
    hs, cs = torch.stack(hs, 1), torch.stack(cs, 1)
    out = {"h_seq": _np64(hs), "c_seq": _np64(cs)}
    if dh is not None:
        dgx, dwh = torch.autograd.grad((hs * dh.detach().cpu().to(dtype)).sum(), (gx, wh))
        out.update(dgx=_np64(dgx), dwh=_np64(dwh))
    return out


def err_of(got, ref):
    """max |got - ref| / max |ref| (an all-zero reference: the absolute error)."""
    got, ref = _np64(got), _np64(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite values"
    norm = float(np.abs(ref).max())
    return float(np.abs(got - ref).max()) / (norm if norm > 0 else 1.0)


def within(tag, got, ref, yard, margin=MARGIN):
    """|got - ref| <= margin max(yardstick, 4 2^-24) max |ref| over every element; prints the figures, returns the error as a
    multiple of max(yardstick, floor).  A reference that is zero everywhere demands exact zeros."""
    err, norm = err_of(got, ref), float(np.abs(_np64(ref)).max())
    if norm == 0:
        print("%s: reference exactly 0, largest |value| %.3e" % (tag, err))
        assert err == 0, "%s: the reference is exactly 0, got up to %.3e" % (tag, err)
        return 0.0
    tol = margin * max(yard, FLOOR)
    print("%s: err %.3e  yardstick %.3e  bound %.3e (margin %d)  max|ref| %.3e  -> %.2f of the bound"
          % (tag, err, yard, tol, margin, norm, err / tol))
    assert err <= tol, "%s: %.3e exceeds %d x max(%.3e, 4 x 2^-24) = %.3e (of max |ref| = %.3e)" % (tag, err, margin, yard, tol, norm)
    return err / max(yard, FLOOR)


ABI_OUTPUTS = ("h_seq", "c_seq", "dgx")


@functools.lru_cache(maxsize=None)
def reference(shape, scale=1.0, seed=0):
    """(oracle, yardstick) of a raw-ABI case: computed once, shared, never modified."""
    t = inputs(shape, scale, seed)
    ref = oracle(t["gx"], t["wh"], t["dh"])
    cpu = loop(t["gx"], t["wh"], t["dh"])
    return ref, {k: err_of(cpu[k], ref[k]) for k in ("h_seq", "c_seq", "dgx", "dwh")}


# ---------------------------------------------------------------- the layer through gan._SigmoidLSTM
MODULE_OUTPUTS = ("y", "dx", "dWx", "db", "dWh")


def module_inputs(case):
    B, T, Fin, U = case
    g = _gen(3, *case)
    torch.manual_seed(sum(case))
    m = gan._SigmoidLSTM(Fin, U)
    with torch.no_grad():
        m.wh.weight.copy_((torch.rand(4 * U, U, generator=g) * 2 - 1) * (2.0 / U ** 0.5))
    return m, torch.randn(B, T, Fin, generator=g), torch.randn(B, T, U, generator=g)


def module_run(m, x, w, device="cpu", dtype=F32):
    """y, dx, dWx, db, dWh of sum(y w) through the module as it dispatches on (device, dtype)."""
    import copy
    m = copy.deepcopy(m).to(device=device, dtype=dtype)
    x = x.to(device=device, dtype=dtype).requires_grad_(True)
    y = m(x)
    gr = torch.autograd.grad((y * w.to(device=device, dtype=dtype)).sum(), [x, m.wx.weight, m.wx.bias, m.wh.weight])
    return dict(zip(MODULE_OUTPUTS, [y.detach()] + list(gr)))


@functools.lru_cache(maxsize=None)
def module_reference(case):
    """(module, x, w, float64 results of the module's loop, yardstick = its fp32 CPU loop against them)."""
    m, x, w = module_inputs(case)
    ref = module_run(m, x, w, dtype=F64)
    cpu = module_run(m, x, w)
    return m, x, w, ref, {k: err_of(cpu[k], ref[k]) for k in MODULE_OUTPUTS}


# ================================================================ tests
@pytest.mark.parametrize("case", [(3, 5, 7, 3), (4, 9, 6, 8), (2, 1, 4, 64), (5, 2, 3, 1)])
def test_oracle_is_float64_autograd_of_the_modules_own_loop(case):
    B, T, Fin, U = case
    m, x, w = module_inputs(case)
    m = m.double()
    x = x.double().requires_grad_(True)
    kept = []
    hook = m.wx.register_forward_hook(lambda mod, args, out: (out.retain_grad(), kept.append(out))[0])   # gx of the module's own call
    y = m(x)
    hook.remove()
    gx, = kept
    (y * w.double()).sum().backward()
    ref = oracle(gx, m.wh.weight, w)
    for tag, got, want in (("h_seq", y, ref["h_seq"]), ("dgx", gx.grad, ref["dgx"]), ("dwh", m.wh.weight.grad, ref["dwh"])):
        e = err_of(got, want)
        print("oracle vs float64 autograd %s %s: %.2e" % (case, tag, e))
        assert e <= 64 * 2.0 ** -53, (tag, e)
    lp = loop(gx, m.wh.weight, w, dtype=F64)            # the helper loop is the module's loop, and gives the cell state too
    assert np.array_equal(lp["h_seq"], _np64(y)) and np.array_equal(lp["dgx"], _np64(gx.grad))
    assert err_of(lp["c_seq"], ref["c_seq"]) <= 64 * 2.0 ** -53
    assert m.wx.weight.grad is not None and x.grad is not None


def test_oracle_gradient_against_central_differences():
    t = inputs((2, 4, 3), seed=5)
    gx, wh, dh = (_np64(t[k]) for k in ("gx", "wh", "dh"))
    ref = oracle(gx, wh, dh)
    loss = lambda a, b: float((oracle(a, b)["h_seq"] * dh).sum())
    eps = 1e-6
    for arr, grad, other in ((gx, ref["dgx"], "gx"), (wh, ref["dwh"], "wh")):
        for idx in list(np.ndindex(arr.shape))[::5]:
            p, q = arr.copy(), arr.copy()
            p[idx] += eps
            q[idx] -= eps
            num = (loss(p, wh) - loss(q, wh)) / (2 * eps) if other == "gx" else (loss(gx, p) - loss(gx, q)) / (2 * eps)
            assert abs(num - grad[idx]) <= 1e-8 + 1e-6 * abs(grad[idx]), (other, idx, num, grad[idx])


@pytest.mark.parametrize("shape,scale", [(TRAINER, 1.0), ((5, 6, 3), 1.0), (SATURATED, 20.0)])
def test_yardstick_is_a_few_fp32_roundings(shape, scale):
    ref, yard = reference(shape, scale)
    print("yardstick %s x%g: %s" % (shape, scale, {k: "%.2e" % v for k, v in yard.items()}))
    assert all(0 <= v < 1e-5 for v in yard.values())
    assert all(np.isfinite(ref[k]).all() for k in ref)


def test_saturated_case_saturates():
    ref, _ = reference(SATURATED, 20.0)
    t = inputs(SATURATED, 20.0)
    assert float((t["gx"].abs() > 17).float().mean()) > 0.3            # sigmoid rounds to 0 or 1 in fp32 there
    assert float(np.abs(ref["dgx"]).max()) > 0


def _header():
    text = open(os.path.join(ROOT, "include", "kccot_models.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_models_header_is_strict_c99(tmp_path):
    gcc = shutil.which("gcc")
    if not gcc:
        pytest.skip("no gcc")
    probe = tmp_path / "hdr.c"
    probe.write_text('#include "kccot_models.h"\nint main(void) { return 0; }\n')
    r = subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only",
                        str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_library_exports_the_model_symbols_and_the_table_matches_the_header():
    from kccotgan_amd import _lib
    decls = dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _header()))
    assert sorted(decls) == ["kccot_sigmoid_lstm_bwd_f32", "kccot_sigmoid_lstm_fwd_f32"]
    assert sorted(_lib.MODEL_SIGNATURES) == sorted(decls), "ctypes table and header disagree"
    assert not set(_lib.MODEL_SIGNATURES) & set(_lib.SIGNATURES)
    ctype = {"int": ctypes.c_int, "kccot_stream_t": ctypes.c_void_p}
    for name, args in decls.items():
        assert hasattr(_lib.lib, name), "libkccot.so does not export %s" % name
        want = []
        for a in args.split(","):
            a = " ".join(a.split())
            want.append(ctypes.c_void_p if "*" in a else ctype[a.rsplit(" ", 1)[0]])
        res, argtypes = _lib.MODEL_SIGNATURES[name]
        assert res is ctypes.c_int and argtypes == want, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want
    assert _lib.lib.kccot_version() == 301                            # the versioned surface is untouched


def test_argument_validation_happens_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)       # never dereferenced: every call below is rejected on its arguments
    fwd, bwd = lib.kccot_sigmoid_lstm_fwd_f32, lib.kccot_sigmoid_lstm_bwd_f32
    for args in ((None, one, 2, 3, 8, one, one), (one, None, 2, 3, 8, one, one), (one, one, 2, 3, 8, None, one)):
        assert fwd(*args, None) == _lib.EINVAL and b"null" in lib.kccot_last_error()
    for shape in ((0, 3, 8), (2, 0, 8), (2, 3, 0), (-1, 3, 8)):
        assert fwd(one, one, *shape, one, None, None) == _lib.EINVAL and b"bad shape" in lib.kccot_last_error()
        assert bwd(one, one, one, one, one, *shape, one, None) == _lib.EINVAL and b"bad shape" in lib.kccot_last_error()
    for k in range(6):              # every pointer of the backward is required
        ptrs = [one] * 6
        ptrs[k] = None
        assert bwd(*ptrs[:5], 2, 3, 8, ptrs[5], None) == _lib.EINVAL and b"null" in lib.kccot_last_error()
    assert fwd(one, one, 2, 3, 65, one, None, None) == _lib.EUNSUPPORTED and b"at most 64" in lib.kccot_last_error()
    assert bwd(one, one, one, one, one, 2, 3, 65, one, None) == _lib.EUNSUPPORTED


def test_dispatch_keeps_the_loop_off_the_gpu_and_the_parameter_names(monkeypatch):
    """CPU tensors, double precision and the switch take the tensor-op loop; state_dict keys are the parent's."""
    m, x, w = module_inputs((3, 5, 7, 3))
    assert sorted(m.state_dict()) == ["wh.weight", "wx.bias", "wx.weight"]
    assert isinstance(gan._SLSTM_HIP, bool)
    a = module_run(m, x, w)
    monkeypatch.setattr(gan, "_SLSTM_HIP", False)
    b = module_run(m, x, w)
    assert all(torch.equal(a[k], b[k]) for k in MODULE_OUTPUTS)
    with pytest.raises(Exception):                      # the Function itself has no CPU path
        gan._SigmoidLSTMHIP.apply(torch.zeros(1, 2, 4), torch.zeros(4, 1))
