"""CPU-side checks of the sigma gradient of the kernel smoothing (include/kccot_smooth_sigma.h; not reference behaviour): the
header against the ctypes table, the header as strict C99, the untouched versioned surface, the argument rules that are decided
before any launch (pointers that are never dereferenced), the fp64 oracle of the GPU tests against finite differences, and the
Python path's refusal of CPU tensors."""
import ctypes
import inspect
import os
import re
import subprocess

import pytest
import torch

import smooth_sigma_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kccot_smooth_dsigma_f32", "kccot_smooth_dsigma_plan", "kccot_smooth_dsigma_workspace_bytes"]


def _decls(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(2), (m.group(1), m.group(3)))
                for m in re.finditer(r"\b(int|size_t)\s+(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_and_ctypes_table_agree_and_the_table_is_disjoint_from_the_others():
    from kccotgan_amd import _lib
    decls = _decls("kccot_smooth_sigma.h")
    assert sorted(decls) == NAMES
    assert sorted(_lib.SMOOTH_SIGMA_SIGNATURES) == NAMES, "ctypes table and header disagree"
    others = [getattr(_lib, n) for n in dir(_lib) if n.endswith("SIGNATURES") and n != "SMOOTH_SIGMA_SIGNATURES"]
    assert len(others) >= 6
    for table in others:
        assert not set(_lib.SMOOTH_SIGMA_SIGNATURES) & set(table)
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t}
    for name, (ret, args) in decls.items():
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        res, argtypes = _lib.SMOOTH_SIGMA_SIGNATURES[name]
        assert res is ctype[ret] and argtypes == want, name
        fn = getattr(_lib.lib, name)                       # bound in the loader's loop
        assert fn.restype is ctype[ret] and list(fn.argtypes) == want


def test_header_compiles_as_strict_c99(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_smooth_sigma.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(probe), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_versioned_surface_is_untouched():
    from kccotgan_amd import _lib
    assert _lib.lib.kccot_version() == 301
    text = open(os.path.join(ROOT, "include", "kccot.h")).read()
    assert "dsigma" not in text and "smooth_sigma" not in text
    assert not [n for n in _lib.SIGNATURES if "dsigma" in n]
    # what kccot.h declares is in the main table, and the new names are in neither
    assert set(_decls("kccot.h")) <= set(_lib.SIGNATURES) and not set(NAMES) & set(_decls("kccot.h"))
    assert _lib.SMOOTH_SIGMA_SIGNATURES and hasattr(_lib.lib, "kccot_smooth_dsigma_f32")


def test_argument_rules_return_their_codes_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is rejected on its arguments
    big = 1 << 30
    T_, H_, W_, CT = _lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W, _lib.SMOOTH_CAUSAL_T
    THW = T_ | H_ | W_

    def ds(flags=THW, x=one, g=one, out=one, mx=one, stats=None, shape=(2, 8, 9, 8, 1), sigma=5.0, r=3, res=one, ws=one,
           wsb=big):
        return lib.kccot_smooth_dsigma_f32(x, g, out, mx, stats, *shape, sigma, r, flags, res, ws, wsb, None)

    # null pointers (stats_in may be null)
    for kw in ("x", "g", "out", "mx", "res"):
        assert ds(**{kw: None}) == _lib.EINVAL, kw
    # shape, sigma, radius
    for shape in ((0, 8, 9, 8, 1), (2, 0, 9, 8, 1), (2, 8, 0, 8, 1), (2, 8, 9, 0, 1), (2, 8, 9, 8, 0)):
        assert ds(shape=shape) == _lib.EINVAL
    assert ds(sigma=0.0) == _lib.EINVAL and ds(sigma=-1.0) == _lib.EINVAL and ds(sigma=float("nan")) == _lib.EINVAL
    assert ds(r=8) == _lib.EINVAL and ds(r=-1) == _lib.EINVAL
    # radius >= the length of a REFLECT axis, for the forms that have that axis
    for flags, shape, code in ((THW, (2, 3, 9, 8, 1), _lib.EINVAL), (THW, (2, 8, 3, 8, 1), _lib.EINVAL),
                               (THW, (2, 8, 9, 3, 1), _lib.EINVAL), (H_ | W_, (2, 3, 9, 8, 1), _lib.EINVAL),
                               (H_ | W_, (2, 8, 9, 3, 1), _lib.EINVAL), (T_, (2, 8, 3, 8, 1), _lib.EINVAL),
                               (THW | CT, (2, 3, 9, 8, 1), _lib.EINVAL), (THW | CT, (2, 8, 9, 3, 1), _lib.EINVAL)):
        assert ds(flags=flags, shape=shape) == code, (flags, shape)
        assert b"REFLECT" in lib.kccot_last_error()
    # an axis that is not smoothed may be short; a causal T has no padding (T = 1 included): as far as the workspace check
    assert ds(flags=H_ | W_, shape=(2, 8, 2, 8, 1), wsb=16) == _lib.EWORKSPACE
    assert ds(flags=T_, shape=(2, 2, 9, 2, 1), wsb=16) == _lib.EWORKSPACE
    assert ds(flags=T_ | CT, shape=(2, 8, 2, 8, 1), wsb=16) == _lib.EWORKSPACE
    assert ds(flags=THW | CT, shape=(2, 8, 1, 8, 1), r=7, wsb=16) == _lib.EWORKSPACE
    # flags: CAUSAL_T without T, a protocol bit, an unknown bit -- EINVAL, the flag named
    for flags, word in ((CT, b"KCCOT_SMOOTH_CAUSAL_T"), (CT | H_ | W_, b"KCCOT_SMOOTH_CAUSAL_T"),
                        (THW | _lib.SMOOTH_NO_DIVIDE, b"KCCOT_SMOOTH_NO_DIVIDE"),
                        (THW | _lib.SMOOTH_EXTERNAL_MAX, b"KCCOT_SMOOTH_EXTERNAL_MAX"),
                        (THW | _lib.SMOOTH_STATS_ONLY, b"KCCOT_SMOOTH_STATS_ONLY"),
                        (T_ | _lib.SMOOTH_EXTERNAL_STATS, b"KCCOT_SMOOTH_EXTERNAL_STATS"), (THW | 256, b"0x107")):
        assert ds(flags=flags) == _lib.EINVAL, flags
        assert word in lib.kccot_last_error(), lib.kccot_last_error()
    # workspace
    need = lib.kccot_smooth_dsigma_workspace_bytes(2, 8, 9, 8, 1)
    assert need > 0 and need % 4 == 0
    assert ds(wsb=need - 1) == _lib.EWORKSPACE and ds(ws=None) == _lib.EWORKSPACE
    assert ds(wsb=need - 1, stats=one) == _lib.EWORKSPACE
    for shape in ((0, 8, 9, 8, 1), (2, 8, 9, 8, 0)):
        assert lib.kccot_smooth_dsigma_workspace_bytes(*shape) == 0


def test_workspace_query_covers_small_and_large_shapes():
    """The partial area is one fp64 per workgroup of the largest grid of any plan: it grows with the tensor and never
    vanishes; the query is a pure function of the shape."""
    from kccotgan_amd import _lib
    q = _lib.lib.kccot_smooth_dsigma_workspace_bytes
    small, mid, large = q(1, 16, 8, 64, 1), q(2, 64, 30, 64, 1), q(16, 64, 30, 64, 3)
    assert 0 < small <= mid <= large
    assert q(2, 64, 30, 64, 1) == mid and q(1, 16, 8, 64, 1) == small       # (the one-entry plan cache does not leak)
    assert large < 16 * 64 * 30 * 64 * 3 * 4, "no tensor-sized intermediate"


@pytest.mark.parametrize("form", so.FORMS)
@pytest.mark.parametrize("r", [1, 3])
@pytest.mark.parametrize("sigma", [0.7, 2.0])
def test_oracle_matches_the_central_finite_difference(form, r, sigma):
    """The analytic dsigma of the oracle equals the central difference of sum g * out in fp64 to 1e-7 relative (tie-free
    input: the arg-max does not move within the step)."""
    gen = torch.Generator().manual_seed(1234 + 10 * r + so.FORMS.index(form))
    x = torch.rand((2, 6, 7, 6, 2), generator=gen, dtype=torch.float64)
    g = torch.randn((2, 6, 7, 6, 2), generator=gen, dtype=torch.float64)
    s, _ = so.fields(x, sigma, r, form)
    mx = s.max()
    out = s / mx
    assert int((out == 1.0).sum()) == 1
    ana, y = so.dsigma_ref(x, g, out, mx, sigma, r, form, round32=False)
    # the five-point central difference: at |dsigma| ~ 1e-4 Y (the derivative taps sum to zero) the h^2 term of the
    # three-point one is 1e-7 of the value by itself; here truncation (h^4) and rounding (1e-16 |loss| / h) are both ~1e-10
    h = 1e-3 * sigma
    f = lambda k: so.loss64(x, g, sigma + k * h, r, form)
    fd = (-f(2) + 8 * f(1) - 8 * f(-1) + f(-2)) / (12 * h)
    print("form %s r %d sigma %g: analytic %.12e fd %.12e Y %.3e" % (form, r, sigma, ana, fd, y))
    assert abs(ana - fd) <= 1e-7 * abs(fd), (ana, fd)
    assert abs(ana) <= y


def test_oracle_derivative_taps_sum_to_zero_and_match_their_finite_difference():
    for sigma in (0.7, 2.0, 5.0):
        for r in (1, 3, 7):
            w, dw = so.sym_taps(sigma, r)
            assert abs(float(dw.sum())) < 1e-15 and abs(float(w.sum()) - 1) < 1e-15
            h = 1e-6 * sigma
            fd = (so.sym_taps(sigma + h, r)[0] - so.sym_taps(sigma - h, r)[0]) / (2 * h)
            assert float((fd - dw).abs().max()) < 1e-8
            V, dV = so.causal_taps(sigma, r, 10)
            assert float(dV.sum(1).abs().max()) < 1e-15 and float(V[0, 0]) == 1.0 and float(dV[0].abs().max()) == 0.0
            fdV = (so.causal_taps(sigma + h, r, 10)[0] - so.causal_taps(sigma - h, r, 10)[0]) / (2 * h)
            assert float((fdV - dV).abs().max()) < 1e-8


def test_a_learnable_sigma_on_cpu_tensors_is_refused():
    from kccotgan_amd import _lib
    from kccotgan_amd.data_utils import KernelSmoothing
    ks = KernelSmoothing(6, 6)
    x = torch.rand(2, 8, 9, 8, 1)
    sigma = torch.tensor(1.3, requires_grad=True)
    for name in ("temporal_convolution", "causal_temporal_convolution", "spatial_convolution", "gaussian_convolution3D",
                 "causal_gaussian_convolution3D"):
        with pytest.raises(_lib.KccotError):
            getattr(ks, name)(x, sigma)
    # the sigma tensor itself is checked before anything else
    with pytest.raises(ValueError):
        ks.temporal_convolution(x, torch.tensor([1.0, 2.0], requires_grad=True))


def test_signatures_and_the_float_path_are_as_before():
    from kccotgan_amd import data_utils as d
    for name in ("temporal_convolution", "causal_temporal_convolution", "spatial_convolution", "gaussian_convolution3D",
                 "causal_gaussian_convolution3D"):
        assert [p for p in inspect.signature(getattr(d.KernelSmoothing, name)).parameters][1:] == ["inputs", "sigma"]
    assert [p for p in inspect.signature(d.KernelSmoothing._apply).parameters][1:] == ["inputs", "sigma", "radius", "axes"]
    # a float sigma and a tensor sigma without requires_grad reach the old functions with a Python float
    ks = d.KernelSmoothing(6, 8)
    seen = []

    class Probe:
        @staticmethod
        def apply(*a):
            seen.append(a[1:])

    saved = d._Smooth, d._SmoothSigma, d._video
    d._Smooth, d._SmoothSigma, d._video = Probe, None, lambda v: v
    try:
        ks.temporal_convolution(None, 2.5)
        ks.gaussian_convolution3D(None, torch.tensor(0.5))
        ks.spatial_convolution(None, torch.tensor(0.25, dtype=torch.float64))
    finally:
        d._Smooth, d._SmoothSigma, d._video = saved
    assert seen == [(2.5, 3, 1), (0.5, 4, 7), (0.25, 4, 6)] and all(type(s[0]) is float for s in seen)
    assert "hipGraph" in d._SmoothSigma.__doc__ and "PARTIAL" in d._SmoothShardedSigma.__doc__
