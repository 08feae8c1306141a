"""CPU-side checks of the per-frame SSIM / PSNR metrics (include/kccot_metrics.h; not reference behaviour): the header against
the ctypes table, the header as strict C99, the untouched versioned surface, the argument rules that are decided before any launch
(pointers that are never dereferenced), the workspace query, the Python path's refusals, the trainer's entry point, and the
oracle of the GPU tests (tests/ssim_oracle.py): against autograd, scipy, and, in float32, against itself in float64 under the
caps the GPU tests may not exceed."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ssim_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kccot_ssim_bwd_f32", "kccot_ssim_fwd_f32", "kccot_ssim_plan", "kccot_ssim_workspace_bytes"]


def _decls(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(2), (m.group(1), m.group(3)))
                for m in re.finditer(r"\b(int|size_t)\s+(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_and_ctypes_table_agree_and_the_table_is_disjoint_from_the_others():
    from kccotgan_amd import _lib
    decls = _decls("kccot_metrics.h")
    assert sorted(decls) == NAMES
    assert sorted(_lib.METRICS_SIGNATURES) == NAMES, "ctypes table and header disagree"
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "METRICS_SIGNATURES"]
    assert len(others) >= 8
    for table in others:
        assert not set(_lib.METRICS_SIGNATURES) & set(table)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t}
    for name, (ret, args) in decls.items():
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        res, argtypes = _lib.METRICS_SIGNATURES[name]
        assert res is ctype[ret] and argtypes == want, name
        fn = getattr(_lib.lib, name)                       # bound in the loader's loop
        assert fn.restype is ctype[ret] and list(fn.argtypes) == want
    # the versioned surface does not know the new names
    assert not set(NAMES) & set(_decls("kccot.h")) and not set(NAMES) & set(_lib.SIGNATURES)
    assert "ssim" not in open(os.path.join(ROOT, "include", "kccot.h")).read()


def test_header_compiles_as_strict_c99(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_metrics.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _callers():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one, two, far = ctypes.c_void_p(16), ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 40)   # never dereferenced
    base = dict(shape=(2, 16, 3, 16, 1), sigma=1.5, r=5, L=1.0, ws=one, wsb=1 << 30)

    def fwd(**kw):
        a = dict(base, x=one, y=two, s=one, m=one)
        a.update(kw)
        return lib.kccot_ssim_fwd_f32(a["x"], a["y"], *a["shape"], a["sigma"], a["r"], a["L"], a["s"], a["m"], a["ws"], a["wsb"],
                                      None)

    def bwd(**kw):
        a = dict(base, g=one, x=one, y=two, dy=far)
        a.update(kw)
        return lib.kccot_ssim_bwd_f32(a["g"], a["x"], a["y"], *a["shape"], a["sigma"], a["r"], a["L"], a["dy"], a["ws"], a["wsb"],
                                      None)

    return _lib, {"fwd": fwd, "bwd": bwd}


def test_argument_rules_return_their_codes_before_any_launch():
    _lib, call = _callers()
    lib = _lib.lib
    for name, kws in (("fwd", ("x", "y", "s")), ("bwd", ("g", "x", "y", "dy"))):
        for kw in kws:
            assert call[name](**{kw: None}) == _lib.EINVAL, (name, kw)
            assert b"null" in lib.kccot_last_error()
    # mse_out alone may be NULL: such a call gets as far as the workspace check
    assert call["fwd"](m=None, wsb=16) == _lib.EWORKSPACE
    for name, f in call.items():
        for k in range(5):
            for bad in (0, -3):
                shape = list((2, 16, 3, 16, 1))
                shape[k] = bad
                assert f(shape=tuple(shape)) == _lib.EINVAL, (name, shape)
                assert b"shape" in lib.kccot_last_error()
        for bad in (0.0, -1.0, float("nan")):
            assert f(sigma=bad) == _lib.EINVAL and b"sigma" in lib.kccot_last_error(), (name, bad)
            assert f(L=bad) == _lib.EINVAL and b"data_range" in lib.kccot_last_error(), (name, bad)
        for bad in (8, -1):
            assert f(r=bad) == _lib.EINVAL and b"radius" in lib.kccot_last_error(), (name, bad)
        # 2 radius >= H or >= W; 2 radius = H - 1 is the 1 x 1 map and passes as far as the workspace
        for shape, r in (((2, 10, 3, 16, 1), 5), ((2, 16, 3, 10, 1), 5), ((2, 16, 3, 9, 1), 5), ((2, 1, 3, 16, 1), 1)):
            assert f(shape=shape, r=r) == _lib.EINVAL and b"does not fit" in lib.kccot_last_error(), (name, shape)
        assert f(shape=(2, 11, 3, 11, 1), r=5, wsb=16) == _lib.EWORKSPACE, name
        assert f(shape=(2, 1, 3, 1, 1), r=0, wsb=16) == _lib.EWORKSPACE, name
        # workspace: null, and the boundary at need - 1
        need = lib.kccot_ssim_workspace_bytes(2, 16, 3, 16, 1)
        assert need > 0 and need % 4 == 0
        assert f(wsb=need - 1) == _lib.EWORKSPACE and b"workspace" in lib.kccot_last_error(), name
        assert f(ws=None) == _lib.EWORKSPACE, name
        # too large to index: B * T above 2^31 - 1 (a dy beyond the 2^42 bytes of such an x and y)
        kw = {"dy": ctypes.c_void_p(1 << 62)} if name == "bwd" else {}
        assert f(shape=(1 << 20, 16, 1 << 12, 16, 1), **kw) == _lib.EUNSUPPORTED and b"too large" in lib.kccot_last_error(), name
    # dy overlapping x or y (the tensor is 2*16*3*16 floats = 6144 bytes)
    x, y = 1 << 20, 1 << 21
    for dy in (x, y, x + 4, y - 4, x + 6140, y - 6140):
        rc = call["bwd"](x=ctypes.c_void_p(x), y=ctypes.c_void_p(y), dy=ctypes.c_void_p(dy))
        assert rc == _lib.EINVAL and b"alias" in lib.kccot_last_error(), dy
    assert call["bwd"](x=ctypes.c_void_p(x), y=ctypes.c_void_p(y), dy=ctypes.c_void_p(x + 6144), wsb=16) == _lib.EWORKSPACE


def test_workspace_query_is_zero_for_bad_shapes_monotone_in_b_and_small():
    from kccotgan_amd import _lib
    q = _lib.lib.kccot_ssim_workspace_bytes
    for k in range(5):
        for bad in (0, -1):
            shape = [2, 16, 3, 16, 1]
            shape[k] = bad
            assert q(*shape) == 0
    for H, T, W, C in ((64, 30, 64, 1), (64, 30, 64, 3), (13, 2, 70, 3), (70, 2, 13, 2), (1, 1, 1, 1), (16, 4, 16, 40)):
        sizes = [q(B, H, T, W, C) for B in (1, 2, 3, 4, 7, 8, 9, 16, 17, 63, 64, 65, 256)]
        assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])), (H, T, W, C, sizes)
        assert q(1, H, T, W, C) == sizes[0]                 # a pure function of the shape
    assert q(256, 64, 30, 64, 3) < 256 * 64 * 30 * 64 * 3 * 4 // 100, "nothing tensor-sized"


def test_python_side_refusals():
    from kccotgan_amd import _lib, metrics
    x, y = so.noise((2, 16, 3, 16, 1), 1)
    for fn in (metrics.ssim, metrics.frame_metrics):
        for win in (2, 10, 0, -1, 17, 4.5):
            with pytest.raises(ValueError, match="win_size"):
                fn(x, y, win_size=win)
        with pytest.raises(ValueError, match="does not fit"):
            fn(x[:, :9], y[:, :9])
        with pytest.raises(ValueError, match="does not fit"):
            fn(x[:, :, :, :9], y[:, :, :, :9])
        with pytest.raises(ValueError, match="one shape"):
            fn(x, y[:1])
        for kw in ({"sigma": 0.0}, {"sigma": float("nan")}, {"data_range": 0.0}, {"data_range": -1.0}):
            with pytest.raises(ValueError, match="> 0"):
                fn(x, y, **kw)
        # no CPU path
        with pytest.raises(_lib.KccotError):
            fn(x, y)
    with pytest.raises(_lib.KccotError):
        metrics.psnr(x, y)
    with pytest.raises(_lib.KccotError):
        metrics.ssim(x, y.clone().requires_grad_(True), win_size=3)
    sig = lambda f: [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    assert sig(metrics.ssim) == sig(metrics.frame_metrics) == [("real", inspect.Parameter.empty), ("fake", inspect.Parameter.empty),
                                                              ("data_range", 1.0), ("win_size", 11), ("sigma", 1.5)]
    assert sig(metrics.psnr) == [("real", inspect.Parameter.empty), ("fake", inspect.Parameter.empty), ("data_range", 1.0)]


def test_trainer_has_evaluate_with_the_stated_signature():
    from kccotgan_amd.kernel_train import KCCOTTrainer
    params = list(inspect.signature(KCCOTTrainer.evaluate).parameters.values())
    assert [(p.name, p.default) for p in params[1:]] == [("test_data", inspect.Parameter.empty), ("data_range", 1.0),
                                                         ("win_size", 11), ("ssim_sigma", 1.5)]
    assert "rank" in KCCOTTrainer.evaluate.__doc__ and "pred_time_steps" in KCCOTTrainer.evaluate.__doc__


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
ORACLE_CASES = [((2, 8, 3, 9, 1), 1, 1.5), ((1, 13, 2, 17, 3), 5, 1.5), ((2, 16, 2, 16, 2), 7, 0.5), ((1, 5, 2, 6, 2), 0, 1.5),
                ((1, 11, 2, 11, 1), 5, 1.5)]


@pytest.mark.parametrize("shape,r,sigma", ORACLE_CASES)
def test_oracle_closed_form_adjoint_equals_autograd(shape, r, sigma):
    x, y = (v.double() for v in so.noise(shape, 7))
    g = so.upstream(shape, 8).double()
    yv = y.clone().requires_grad_(True)
    (so.scores(x, yv, sigma, r) * g).sum().backward()
    dy = so.adjoint(g, x, y, sigma, r)
    assert dy.shape == y.shape
    assert float((dy - yv.grad).abs().max()) <= 1e-12 * max(1.0, float(yv.grad.abs().max()))


@pytest.mark.parametrize("shape,r,sigma", ORACLE_CASES)
def test_oracle_identity_symmetry_and_scipy(shape, r, sigma):
    from scipy.ndimage import correlate1d
    x, y = (v.double() for v in so.noise(shape, 9))
    assert float((so.scores(x, x, sigma, r) - 1.0).abs().max()) <= 1e-12
    assert float((so.scores(x, y, sigma, r) - so.scores(y, x, sigma, r)).abs().max()) <= 1e-12
    assert float(so.mse(x, x).abs().max()) == 0.0
    # an independent path: scipy's same-size correlation, cropped to the window positions that lie inside the frame
    w = so.taps(sigma, r).numpy()
    assert abs(w.sum() - 1.0) < 1e-6 and np.array_equal(w, w[::-1])

    def G(v):
        full = correlate1d(correlate1d(v.numpy(), w, axis=3, mode="constant"), w, axis=1, mode="constant")
        return full[:, r:full.shape[1] - r, :, r:full.shape[3] - r, :]

    mx, my = G(x), G(y)
    sxx, syy, sxy = G(x * x) - mx * mx, G(y * y) - my * my, G(x * y) - mx * my
    S = (2 * mx * my + 1e-4) * (2 * sxy + 9e-4) / ((mx * mx + my * my + 1e-4) * (sxx + syy + 9e-4))
    ref = S.mean(axis=(1, 3, 4))
    assert S.shape == tuple(so.ssim_map(x, y, sigma, r).shape)
    assert float(np.abs(so.scores(x, y, sigma, r).numpy() - ref).max()) <= 1e-6
    assert float(np.abs(so.mse(x, y).numpy() - ((x - y).numpy() ** 2).mean(axis=(1, 3, 4))).max()) <= 1e-15


def test_oracle_taps_are_fp32_values_next_to_the_exact_taps():
    """make_taps (csrc/smooth_internal.h): fp32 values, symmetric, within fp32 rounding of the exact normalised Gaussian"""
    for sigma, r in ((1.5, 5), (0.5, 7), (1.5, 1), (5.0, 3), (1.5, 0)):
        w = so.taps(sigma, r)
        d = torch.arange(-r, r + 1, dtype=torch.float64)
        e = torch.exp(-d * d / (2.0 * sigma * sigma))
        assert float((w - e / e.sum()).abs().max()) <= 4e-7
        assert torch.equal(w, w.flip(0)) and all(float(v) == float(np.float32(float(v))) for v in w)
    assert float(so.taps(0.5, 7)[0]) < 1.2e-38              # taps that underflow (below the smallest normal fp32)
    assert float(so.taps(1.5, 0)[0]) == 1.0


@pytest.mark.parametrize("shape,win,sigma,kind", so.GRID, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_the_reference_alone_stays_inside_the_caps(shape, win, sigma, kind):
    """The oracle in float32 against itself in float64 at every shape of the GPU tests: the caps of tests/test_gpu_ssim.py leave
    room for a correct float32 evaluation."""
    r = win // 2
    x, y = so.inputs(kind, shape, 11)
    g = so.upstream(shape, 12)
    ref = so.scores(x.double(), y.double(), sigma, r)
    err = float((so.scores(x, y, sigma, r).double() - ref).abs().max())
    print("%s %s win %d: float32 scores err %.3e" % (kind, shape, win, err))
    assert err <= so.CAP_SSIM[kind]
    if kind == "noise":
        d_ref = so.adjoint(g.double(), x.double(), y.double(), sigma, r)
        d_err = float((so.adjoint(g, x, y, sigma, r).double() - d_ref).abs().max()) / float(d_ref.abs().max())
        print("%s %s win %d: float32 adjoint err / max %.3e" % (kind, shape, win, d_err))
        assert d_err <= so.CAP_DY


@pytest.mark.parametrize("r", range(8))
def test_flat_adjoint_in_float32_stays_inside_the_cap_except_at_radius_0(r):
    """The condition under which tests/test_gpu_tile_instantiations.py bounds the adjoint on the FLAT input by CAP_DY: the oracle
    in float32 against itself in float64, on that module's own inputs (the radius cases of tests/tile_plan_cases.py, seeds 71 and
    72, sigma 1.5).  Radii 1..7 stay inside the cap; radius 0 does not -- one tap of weight 1 makes the three variances
    differences of equal numbers, float32 leaves rounding noise there (the kernel writes exact zeros) -- so the GPU module
    leaves the flat adjoint at radius 0 out."""
    import tile_plan_cases as tp
    shape = tp.SSIM_SHAPE_R
    assert [c[1] for c in tp.SSIM_CASES if "radius" in c[3]] == [shape] * 8
    x, y = so.inputs("flat", shape, 71)
    g = so.upstream(shape, 72)
    ref = so.adjoint(g.double(), x.double(), y.double(), 1.5, r)
    err = float((so.adjoint(g, x, y, 1.5, r).double() - ref).abs().max()) / float(ref.abs().max())
    print("flat %s r %d: float32 adjoint err / max %.3e (cap %.1e)" % (shape, r, err, so.CAP_DY))
    if r == 0:
        assert err > so.CAP_DY, "the flat adjoint at radius 0 can join the GPU module's cases now"
    else:
        assert err <= so.CAP_DY
