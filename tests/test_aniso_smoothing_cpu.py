"""CPU-side checks of the anisotropic 3-D kernel smoothing (include/kccot_smooth_aniso.h; not reference behaviour): the header
against the ctypes table, the header as strict C99, the untouched versioned surface, the argument rules that are decided before
any launch (pointers that are never dereferenced), the workspace query, the fp64 oracle of the GPU tests against finite
differences and autograd, the Python path's refusals and the trainer's routing."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import smooth_aniso_oracle as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kccot_smooth_aniso_bwd_f32", "kccot_smooth_aniso_bwd_sharded_f32", "kccot_smooth_aniso_dsigma_f32",
         "kccot_smooth_aniso_fwd_f32", "kccot_smooth_aniso_plan", "kccot_smooth_aniso_workspace_bytes"]


def _decls(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(2), (m.group(1), m.group(3)))
                for m in re.finditer(r"\b(int|size_t)\s+(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_and_ctypes_table_agree_and_the_table_is_disjoint_from_the_others():
    from kccotgan_amd import _lib
    decls = _decls("kccot_smooth_aniso.h")
    assert sorted(decls) == NAMES
    assert sorted(_lib.SMOOTH_ANISO_SIGNATURES) == NAMES, "ctypes table and header disagree"
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "SMOOTH_ANISO_SIGNATURES"]
    assert len(others) >= 7
    for table in others:
        assert not set(_lib.SMOOTH_ANISO_SIGNATURES) & set(table)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t}
    for name, (ret, args) in decls.items():
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        res, argtypes = _lib.SMOOTH_ANISO_SIGNATURES[name]
        assert res is ctype[ret] and argtypes == want, name
        fn = getattr(_lib.lib, name)                       # bound in the loader's loop
        assert fn.restype is ctype[ret] and list(fn.argtypes) == want


def test_header_compiles_as_strict_c99(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_smooth_aniso.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(probe), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_versioned_surface_is_untouched():
    from kccotgan_amd import _lib
    assert _lib.lib.kccot_version() == 301
    assert "aniso" not in open(os.path.join(ROOT, "include", "kccot.h")).read()
    assert not [n for n in _lib.SIGNATURES if "aniso" in n]
    assert set(_decls("kccot.h")) <= set(_lib.SIGNATURES) and not set(NAMES) & set(_decls("kccot.h"))


def _callers():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)   # never dereferenced: every call is rejected on its arguments
    big = 1 << 30
    base = dict(shape=(2, 8, 9, 8, 1), st=1.3, rt=2, ss=5.0, rs=3, flags=0, ws=one, wsb=big)

    def fwd(**kw):
        a = dict(base, x=one, out=ctypes.c_void_p(32), mx=one)
        a.update(kw)
        return lib.kccot_smooth_aniso_fwd_f32(a["x"], *a["shape"], a["st"], a["rt"], a["ss"], a["rs"], a["flags"], a["out"],
                                              a["mx"], a["ws"], a["wsb"], None)

    def bwd(**kw):
        a = dict(base, g=one, out=one, mx=one, din=one)
        a.update(kw)
        return lib.kccot_smooth_aniso_bwd_f32(a["g"], a["out"], a["mx"], *a["shape"], a["st"], a["rt"], a["ss"], a["rs"],
                                              a["flags"], a["din"], a["ws"], a["wsb"], None)

    def shd(**kw):
        a = dict(base, g=one, out=one, mx=one, stats=one, din=one, flags=_lib.SMOOTH_EXTERNAL_STATS)
        a.update(kw)
        return lib.kccot_smooth_aniso_bwd_sharded_f32(a["g"], a["out"], a["mx"], a["stats"], *a["shape"], a["st"], a["rt"],
                                                      a["ss"], a["rs"], a["flags"], a["din"], a["ws"], a["wsb"], None)

    def dsg(**kw):
        a = dict(base, x=one, g=one, out=one, mx=one, stats=None, res=one)
        a.update(kw)
        return lib.kccot_smooth_aniso_dsigma_f32(a["x"], a["g"], a["out"], a["mx"], a["stats"], *a["shape"], a["st"], a["rt"],
                                                 a["ss"], a["rs"], a["flags"], a["res"], a["ws"], a["wsb"], None)

    return _lib, {"fwd": fwd, "bwd": bwd, "shd": shd, "dsg": dsg}


def test_argument_rules_return_their_codes_before_any_launch():
    _lib, call = _callers()
    lib = _lib.lib
    CT, ND, XM, SO, XS = (_lib.SMOOTH_CAUSAL_T, _lib.SMOOTH_NO_DIVIDE, _lib.SMOOTH_EXTERNAL_MAX, _lib.SMOOTH_STATS_ONLY,
                          _lib.SMOOTH_EXTERNAL_STATS)
    shd_flags = lambda f: (f | XS) if not f & (SO | XS) else f      # the sharded backward always carries one stats flag
    # null pointers (dsigma's stats_in may be null; STATS_ONLY takes no din)
    for name, kws in (("fwd", ("x", "out", "mx")), ("bwd", ("g", "out", "mx", "din")),
                      ("shd", ("g", "out", "mx", "stats", "din")), ("dsg", ("x", "g", "out", "mx", "res"))):
        for kw in kws:
            assert call[name](**{kw: None}) == _lib.EINVAL, (name, kw)
    assert call["shd"](flags=SO, din=None, wsb=16) == _lib.EWORKSPACE
    for name, f in call.items():
        fl = shd_flags(0) if name == "shd" else 0
        # shape, sigma, radius
        for shape in ((0, 8, 9, 8, 1), (2, 0, 9, 8, 1), (2, 8, 0, 8, 1), (2, 8, 9, 0, 1), (2, 8, 9, 8, 0)):
            assert f(shape=shape, flags=fl) == _lib.EINVAL, (name, shape)
        for bad in (0.0, -1.0, float("nan")):
            assert f(st=bad, flags=fl) == _lib.EINVAL and f(ss=bad, flags=fl) == _lib.EINVAL, (name, bad)
        for bad in (8, -1):
            assert f(rt=bad, flags=fl) == _lib.EINVAL and f(rs=bad, flags=fl) == _lib.EINVAL, (name, bad)
        # radius_s >= H or >= W; radius_t >= T only when symmetric
        for shape, rt, rs in (((2, 3, 9, 8, 1), 2, 3), ((2, 8, 9, 3, 1), 2, 3), ((2, 8, 2, 8, 1), 2, 3), ((2, 8, 7, 8, 1), 7, 3)):
            assert f(shape=shape, rt=rt, rs=rs, flags=fl) == _lib.EINVAL, (name, shape)
            assert b"REFLECT" in lib.kccot_last_error()
        assert f(shape=(2, 3, 9, 8, 1), flags=fl | CT) == _lib.EINVAL and f(shape=(2, 8, 9, 3, 1), flags=fl | CT) == _lib.EINVAL
        # a causal T has no padding (radius_t >= T, T = 1 included): as far as the workspace check
        assert f(shape=(2, 8, 2, 8, 1), rt=2, flags=fl | CT, wsb=16) == _lib.EWORKSPACE, name
        assert f(shape=(2, 8, 1, 8, 1), rt=7, flags=fl | CT, wsb=16) == _lib.EWORKSPACE, name
        # radius 0 lifts the constraint of its axis group
        assert f(shape=(2, 1, 9, 1, 1), rs=0, flags=fl, wsb=16) == _lib.EWORKSPACE, name
        assert f(shape=(2, 8, 1, 8, 1), rt=0, flags=fl, wsb=16) == _lib.EWORKSPACE, name
        # workspace: null, and the boundary at need - 1
        need = lib.kccot_smooth_aniso_workspace_bytes(2, 8, 9, 8, 1)
        assert need > 0 and need % 4 == 0
        assert f(flags=fl, wsb=need - 1) == _lib.EWORKSPACE and f(flags=fl, ws=None) == _lib.EWORKSPACE, name
        assert b"workspace" in lib.kccot_last_error()
    # in-place forward
    assert call["fwd"](out=ctypes.c_void_p(16)) == _lib.EINVAL and b"in-place" in lib.kccot_last_error()
    # refused flags, named
    refused = {"fwd": (SO, XS), "bwd": (ND, XM, SO, XS), "shd": (ND, XM), "dsg": (ND, XM, SO, XS)}
    word = {ND: b"KCCOT_SMOOTH_NO_DIVIDE", XM: b"KCCOT_SMOOTH_EXTERNAL_MAX", SO: b"KCCOT_SMOOTH_STATS_ONLY",
            XS: b"KCCOT_SMOOTH_EXTERNAL_STATS", _lib.SMOOTH_T: b"KCCOT_SMOOTH_T", _lib.SMOOTH_H: b"KCCOT_SMOOTH_H",
            _lib.SMOOTH_W: b"KCCOT_SMOOTH_W"}
    for name, f in call.items():
        for bit in refused[name] + (_lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W):
            fl = shd_flags(bit) if name == "shd" else bit
            assert f(flags=fl) == _lib.EINVAL, (name, bit)
            assert word[bit] in lib.kccot_last_error(), (name, bit, lib.kccot_last_error())
        fl = shd_flags(256) if name == "shd" else 256
        assert f(flags=fl) == _lib.EINVAL and b"0x100" in lib.kccot_last_error(), name
    # the exclusive pairs
    assert call["fwd"](flags=ND | XM) == _lib.EINVAL and b"exclusive" in lib.kccot_last_error()
    assert call["shd"](flags=SO | XS) == _lib.EINVAL and call["shd"](flags=0) == _lib.EINVAL
    assert call["shd"](flags=CT) == _lib.EINVAL and b"exactly one" in lib.kccot_last_error()
    # accepted flags get as far as the workspace
    for name, fl in (("fwd", ND), ("fwd", XM | CT), ("bwd", CT), ("shd", SO | CT), ("shd", XS), ("dsg", CT)):
        assert call[name](flags=fl, wsb=16) == _lib.EWORKSPACE, (name, fl)
    for shape in ((0, 8, 9, 8, 1), (2, 8, 9, 8, 0)):
        assert lib.kccot_smooth_aniso_workspace_bytes(*shape) == 0


def test_workspace_query_is_positive_monotone_and_small():
    """One slot per workgroup of the largest grid of any plan plus the per-256-element partial sums: it grows with the tensor,
    never vanishes, holds nothing tensor-sized, and is a pure function of the shape."""
    from kccotgan_amd import _lib
    q = _lib.lib.kccot_smooth_aniso_workspace_bytes
    small, mid, large = q(1, 16, 8, 64, 1), q(2, 64, 30, 64, 1), q(16, 64, 30, 64, 3)
    assert 0 < small <= mid <= large
    assert q(2, 64, 30, 64, 1) == mid and q(1, 16, 8, 64, 1) == small       # (the one-entry plan cache does not leak)
    assert large < 16 * 64 * 30 * 64 * 3 * 4, "no tensor-sized intermediate"
    assert q(1, 1, 1, 1, 1) > 0


CASES = [((1, 3), (0.7, 2.0)), ((3, 1), (2.0, 0.7)), ((1, 3), (2.0, 0.7)), ((3, 1), (0.7, 2.0))]


def _case(idx, causal):
    gen = torch.Generator().manual_seed(5001 + 10 * idx + int(causal))   # (seeds whose maximum leads the runner-up by > 5e-3)
    x = torch.rand((2, 6, 7, 6, 2), generator=gen, dtype=torch.float64)
    g = torch.randn((2, 6, 7, 6, 2), generator=gen, dtype=torch.float64)
    return x, g


@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("idx", range(len(CASES)))
def test_oracle_partials_match_the_central_finite_difference(idx, causal):
    """Both analytic partials of the oracle equal the five-point central difference of sum g * out in fp64 to 1e-7 relative
    (tie-free input: the arg-max does not move within the step)."""
    (rt, rs), (st, ss) = CASES[idx]
    x, g = _case(idx, causal)
    out, mx, _ = ao.forward(x, st, ss, rt, rs, causal)
    top = torch.sort(out.flatten()).values
    assert int((out == 1.0).sum()) == 1 and float(top[-1] - top[-2]) > 5e-3
    (dt, ds), (yt, ys) = ao.dsigma_ref(x, g, out, mx, st, ss, rt, rs, causal, round32=False)
    for which, ana, y, sig in (("t", dt, yt, st), ("s", ds, ys, ss)):
        h = 1e-3 * sig
        f = lambda k: ao.loss64(x, g, st + (k * h if which == "t" else 0.0), ss + (k * h if which == "s" else 0.0), rt, rs, causal)
        fd = (-f(2) + 8 * f(1) - 8 * f(-1) + f(-2)) / (12 * h)
        print("r (%d,%d) sigma (%g,%g) causal %d d/dsigma_%s: analytic %.12e fd %.12e Y %.3e" % (rt, rs, st, ss, causal, which, ana, fd, y))
        assert abs(ana - fd) <= 1e-7 * abs(fd), (which, ana, fd)
        assert abs(ana) <= y


_ADJ = [((2, 6, 7, 6, 2), 1, 3), ((2, 6, 7, 6, 2), 3, 1), ((1, 8, 4, 16, 1), 3, 7), ((1, 5, 9, 20, 1), 7, 4), ((1, 3, 5, 4, 1), 0, 2),
        ((1, 3, 5, 4, 1), 2, 0)]


@pytest.mark.parametrize("shape,rt,rs,causal", [c + (False,) for c in _ADJ] + [c + (True,) for c in _ADJ] +
                         [((1, 5, 4, 6, 5), 7, 2, True), ((1, 3, 1, 4, 1), 5, 1, True)])
def test_oracle_adjoint_with_effective_border_taps_equals_autograd(shape, rt, rs, causal):
    """The header's border coefficients: the gather with them equals torch autograd of the oracle forward (fp64) to 1e-12,
    also on axes with no interior (L <= 2r + 1) and with the causal T at radius >= T."""
    gen = torch.Generator().manual_seed(99)
    x = torch.rand(shape, generator=gen, dtype=torch.float64, requires_grad=True)
    u = torch.randn(shape, generator=gen, dtype=torch.float64)
    s = ao.fields(x, 1.3, 2.1, rt, rs, causal)[0]
    (s * u).sum().backward()
    din = ao.adjoint(u, 1.3, 2.1, rt, rs, causal)
    assert float((din - x.grad).abs().max()) <= 1e-12 * max(1.0, float(x.grad.abs().max()))


def test_cpu_tensors_and_a_two_element_learnable_sigma_are_refused():
    from kccotgan_amd import _lib
    from kccotgan_amd.data_utils import KernelSmoothing
    ks = KernelSmoothing(4, 6)
    assert (ks.temporal_radius, ks.spatial_radius) == (2, 3)
    x = torch.rand(2, 8, 9, 8, 1)
    for st, ss in ((1.3, 5.0), (torch.tensor(1.3, requires_grad=True), 5.0), (1.3, torch.tensor([5.0], requires_grad=True))):
        for causal in (False, True):
            with pytest.raises(_lib.KccotError):
                ks.anisotropic_gaussian_convolution3D(x, st, ss, causal=causal)
    # the sigma tensors themselves are checked before anything else
    two = torch.tensor([1.0, 2.0], requires_grad=True)
    with pytest.raises(ValueError, match="sigma_t"):
        ks.anisotropic_gaussian_convolution3D(x, two, 5.0)
    with pytest.raises(ValueError, match="sigma_s"):
        ks.anisotropic_gaussian_convolution3D(x, 1.3, two)
    doc = KernelSmoothing.anisotropic_gaussian_convolution3D.__doc__
    assert "NOT reference behaviour" in doc and "TEMPORAL radius" in doc and "gaussian_convolution3D" in doc


def test_the_method_routes_sigmas_radii_and_the_sharded_form():
    from kccotgan_amd import _lib
    from kccotgan_amd import data_utils as d
    assert [p for p in inspect.signature(d.KernelSmoothing.anisotropic_gaussian_convolution3D).parameters][1:] == [
        "inputs", "sigma_t", "sigma_s", "causal"]
    seen = []

    class Probe:
        @staticmethod
        def apply(*a):
            seen.append(a[1:])

    saved = d._SmoothAniso, d._SmoothAnisoSharded, d._video
    d._SmoothAniso, d._SmoothAnisoSharded, d._video = Probe, Probe, lambda v: v
    learn = torch.tensor(0.5, requires_grad=True)
    try:
        d.KernelSmoothing(6, 8).anisotropic_gaussian_convolution3D(None, 2.5, torch.tensor(0.25, dtype=torch.float64))
        d.KernelSmoothing(4, 6).anisotropic_gaussian_convolution3D(None, learn, 3, causal=True)
        d.KernelSmoothing(6, 6, sharded=True).anisotropic_gaussian_convolution3D(None, 1.0, 2.0)
    finally:
        d._SmoothAniso, d._SmoothAnisoSharded, d._video = saved
    assert seen[0] == (2.5, 0.25, 3, 4, 0) and all(type(s) is float for s in seen[0][:2])
    assert seen[1][0] is learn and seen[1][1:] == (3.0, 2, 3, _lib.SMOOTH_CAUSAL_T) and type(seen[1][1]) is float
    assert seen[2] == (1.0, 2.0, 3, 3, 0, None)
    assert "hipGraph" in d._SmoothAniso.__doc__ and "PARTIALS" in d._SmoothAnisoSharded.__doc__


@pytest.mark.parametrize("kernel,causal", [("3d_aniso", False), ("3d_aniso_causal", True)])
def test_trainer_routes_the_kernel_names_and_refuses_a_sigma_that_is_no_pair(kernel, causal):
    from kccotgan_amd.kernel_train import KCCOTTrainer

    class Probe:
        kernel_choice = kernel

        class gaussian_kernel:
            @staticmethod
            def anisotropic_gaussian_convolution3D(v, sigma_t, sigma_s, causal=False):
                return ("aniso", v, sigma_t, sigma_s, causal)

    assert KCCOTTrainer._smooth(Probe(), "v", (0.5, 2.0)) == ("aniso", "v", 0.5, 2.0, causal)
    assert KCCOTTrainer._smooth(Probe(), "v", [0.5, 2.0]) == ("aniso", "v", 0.5, 2.0, causal)
    for bad in (0.5, (0.5,), (1.0, 2.0, 3.0), None):
        with pytest.raises(ValueError, match=kernel):
            KCCOTTrainer._smooth(Probe(), "v", bad)
    params = list(inspect.signature(KCCOTTrainer.__init__).parameters.values())
    assert [(p.name, p.default) for p in params[-2:]] == [("temporal_kernel_size", 6), ("spatial_kernel_size", 6)]
    assert [p for p in inspect.signature(KCCOTTrainer._smooth).parameters] == ["self", "v", "sigma"]
