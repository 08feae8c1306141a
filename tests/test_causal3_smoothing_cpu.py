"""CPU-side checks of the causal 3-D smoothing (include/kccot_smooth_causal3.h; past-only in time, symmetric in space; not
reference behaviour): the header against the ctypes table, the header as strict C99, the argument rules that are decided before
any launch (pointers that are never dereferenced), the untouched versioned surface, and the Python method's signature."""
import ctypes
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kccot_smooth_causal3_bwd_f32", "kccot_smooth_causal3_bwd_sharded_f32", "kccot_smooth_causal3_fwd_f32"]


def _decls():
    text = open(os.path.join(ROOT, "include", "kccot_smooth_causal3.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(1), m.group(2)) for m in re.finditer(r"\b(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_and_ctypes_table_agree_and_the_table_is_disjoint_from_the_other_three():
    from kccotgan_amd import _lib
    decls = _decls()
    assert sorted(decls) == NAMES
    assert sorted(_lib.SMOOTH3C_SIGNATURES) == NAMES, "ctypes table and header disagree"
    others = set(_lib.SIGNATURES) | set(_lib.MODEL_SIGNATURES) | set(_lib.WEIGHTED_SIGNATURES)
    assert not set(_lib.SMOOTH3C_SIGNATURES) & others
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "unsigned": ctypes.c_uint, "size_t": ctypes.c_size_t}
    for name, args in decls.items():
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        res, argtypes = _lib.SMOOTH3C_SIGNATURES[name]
        assert res is ctypes.c_int and argtypes == want, name
        fn = getattr(_lib.lib, name)                       # bound in the loader's loop
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == want
        # the parameter list of the kccot_smooth_* counterpart
        assert argtypes == _lib.SIGNATURES[name.replace("_causal3", "")][1], name


def test_header_compiles_as_strict_c99(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_smooth_causal3.h"\nint main(void) { return 0; }\n')
    r = subprocess.run(["cc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(probe), "-o", str(tmp_path / "probe.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_versioned_surface_is_untouched():
    from kccotgan_amd import _lib
    assert _lib.lib.kccot_version() == 301
    text = open(os.path.join(ROOT, "include", "kccot.h")).read()
    assert "causal3" not in text
    assert not [n for n in _lib.SIGNATURES if "causal3" in n]


def test_argument_rules_return_their_codes_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is rejected on its arguments
    two = ctypes.c_void_p(32)
    big = 1 << 30
    ST, SX = _lib.SMOOTH_STATS_ONLY, _lib.SMOOTH_EXTERNAL_STATS
    ND, XM = _lib.SMOOTH_NO_DIVIDE, _lib.SMOOTH_EXTERNAL_MAX

    def fwd(flags=0, src=one, dst=two, mx=one, shape=(2, 8, 9, 8, 1), sigma=5.0, r=3, ws=one, wsb=big):
        return lib.kccot_smooth_causal3_fwd_f32(src, *shape, sigma, r, flags, dst, mx, ws, wsb, None)

    def bwd(flags=0, g=one, out=one, mx=one, din=two, shape=(2, 8, 9, 8, 1), sigma=5.0, r=3, ws=one, wsb=big):
        return lib.kccot_smooth_causal3_bwd_f32(g, out, mx, *shape, sigma, r, flags, din, ws, wsb, None)

    def shd(flags=SX, g=one, out=one, mx=one, stats=one, din=two, shape=(2, 8, 9, 8, 1), sigma=5.0, r=3, ws=one, wsb=big):
        return lib.kccot_smooth_causal3_bwd_sharded_f32(g, out, mx, stats, *shape, sigma, r, flags, din, ws, wsb, None)

    # an axis bit, CAUSAL_T or an unknown bit: EINVAL, the entry point named
    for bit in (_lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W, _lib.SMOOTH_CAUSAL_T, _lib.SMOOTH_T | _lib.SMOOTH_H | _lib.SMOOTH_W,
                _lib.SMOOTH_T | _lib.SMOOTH_CAUSAL_T, 256):
        for f, name, extra in ((fwd, b"kccot_smooth_causal3_fwd_f32", 0), (bwd, b"kccot_smooth_causal3_bwd_f32", 0),
                               (shd, b"kccot_smooth_causal3_bwd_sharded_f32", SX),
                               (shd, b"kccot_smooth_causal3_bwd_sharded_f32", ST)):
            assert f(flags=bit | extra) == _lib.EINVAL, (bit, name)
            assert name in lib.kccot_last_error(), lib.kccot_last_error()
    # null pointers
    assert fwd(src=None) == _lib.EINVAL and fwd(dst=None) == _lib.EINVAL and fwd(mx=None) == _lib.EINVAL
    assert bwd(g=None) == _lib.EINVAL and bwd(out=None) == _lib.EINVAL and bwd(mx=None) == _lib.EINVAL and bwd(din=None) == _lib.EINVAL
    assert shd(stats=None) == _lib.EINVAL and shd(din=None) == _lib.EINVAL and shd(flags=ST, stats=None) == _lib.EINVAL
    # shape, sigma, radius
    for f in (fwd, bwd, shd):
        for shape in ((0, 8, 9, 8, 1), (2, 0, 9, 8, 1), (2, 8, 0, 8, 1), (2, 8, 9, 0, 1), (2, 8, 9, 8, 0)):
            assert f(shape=shape) == _lib.EINVAL
        assert f(sigma=0.0) == _lib.EINVAL and f(sigma=-1.0) == _lib.EINVAL
        assert f(r=8) == _lib.EUNSUPPORTED and f(r=-1) == _lib.EUNSUPPORTED
        assert f(shape=(2, 3, 9, 8, 1)) == _lib.EINVAL       # r >= H
        assert f(shape=(2, 8, 9, 3, 1)) == _lib.EINVAL       # r >= W
        assert b"REFLECT" in lib.kccot_last_error()
        # r >= T is fine (no padding along T): the call gets as far as the workspace check
        assert f(shape=(2, 8, 2, 8, 1), wsb=16) == _lib.EWORKSPACE
        assert f(shape=(2, 8, 1, 8, 1), r=7, wsb=16) == _lib.EWORKSPACE
        need = lib.kccot_smooth_workspace_bytes(2, 8, 9, 8, 1)
        assert f(wsb=need - 1) == _lib.EWORKSPACE and f(ws=None) == _lib.EWORKSPACE
    # exclusivity rules of the symmetric calls
    assert fwd(flags=ND | XM) == _lib.EINVAL
    assert fwd(dst=one) == _lib.EINVAL                       # in place
    assert bwd(flags=ST) == _lib.EINVAL and bwd(flags=SX) == _lib.EINVAL
    assert b"kccot_smooth_causal3_bwd_sharded_f32" in lib.kccot_last_error()
    assert shd(flags=0) == _lib.EINVAL and shd(flags=ST | SX) == _lib.EINVAL
    # STATS_ONLY does not need din
    assert shd(flags=ST, din=None, wsb=16) == _lib.EWORKSPACE


def test_method_exists_with_the_parameters_of_gaussian_convolution3d():
    from kccotgan_amd import data_utils as d
    f = d.KernelSmoothing.causal_gaussian_convolution3D
    assert [p for p in inspect.signature(f).parameters][1:] == ["inputs", "sigma"]
    assert [p for p in inspect.signature(d.KernelSmoothing.gaussian_convolution3D).parameters][1:] == ["inputs", "sigma"]
    assert "NOT reference behaviour" in f.__doc__ and "SPATIAL radius" in f.__doc__
    # the spatial radius, not the temporal one
    ks = d.KernelSmoothing(temporal_kernel_size=6, spatial_kernel_size=8)
    seen = []
    ks._apply = lambda inputs, sigma, radius, axes: seen.append((radius, axes))
    ks.causal_gaussian_convolution3D(None, 1.0)
    assert seen == [(4, d.CAUSAL3)]


def test_trainer_source_routes_the_kernel_name_to_the_method():
    from kccotgan_amd.kernel_train import KCCOTTrainer

    class Probe:
        kernel_choice = "3d_causal"

        class gaussian_kernel:
            @staticmethod
            def causal_gaussian_convolution3D(v, sigma):
                return ("causal3", v, sigma)

    assert KCCOTTrainer._smooth(Probe(), "v", 0.5) == ("causal3", "v", 0.5)
