"""CPU-side checks of KCCOT_SMOOTH_CAUSAL_T (the past-only temporal smoothing; not reference behaviour): the flag's value in
the header and in the ctypes mirror, the Python method's signature, and the argument rules that are decided before any launch."""
import ctypes
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flag_value_in_the_header_and_the_ctypes_mirror():
    from kccotgan_amd import _lib
    text = open(os.path.join(ROOT, "include", "kccot.h")).read()
    m = re.search(r"^#define\s+KCCOT_SMOOTH_CAUSAL_T\s+(\d+)u\s*$", text, flags=re.M)
    assert m, "include/kccot.h does not define KCCOT_SMOOTH_CAUSAL_T"
    assert int(m.group(1)) == 8 and _lib.SMOOTH_CAUSAL_T == 8
    others = [_lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W, _lib.SMOOTH_NO_DIVIDE, _lib.SMOOTH_EXTERNAL_MAX,
              _lib.SMOOTH_STATS_ONLY, _lib.SMOOTH_EXTERNAL_STATS]
    assert all(_lib.SMOOTH_CAUSAL_T & o == 0 for o in others)
    assert _lib.lib.kccot_version() == 301


def test_method_exists_with_the_parameters_of_temporal_convolution():
    from kccotgan_amd import data_utils as d
    f = d.KernelSmoothing.causal_temporal_convolution
    assert [p for p in inspect.signature(f).parameters][1:] == ["inputs", "sigma"]
    assert [p for p in inspect.signature(d.KernelSmoothing.temporal_convolution).parameters][1:] == ["inputs", "sigma"]
    assert "NOT reference behaviour" in f.__doc__


def test_flag_is_rejected_with_h_or_w_or_without_t_before_any_launch():
    from kccotgan_amd import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)   # never dereferenced: every call below is rejected on its arguments
    big = 1 << 30
    Cz, T, H, W = _lib.SMOOTH_CAUSAL_T, _lib.SMOOTH_T, _lib.SMOOTH_H, _lib.SMOOTH_W
    for flags in (Cz | T | H, Cz | T | W, Cz | T | H | W, Cz, Cz | H | W):
        assert lib.kccot_smooth_fwd_f32(one, 2, 8, 9, 8, 1, 5.0, 3, flags, one, one, one, big, None) == _lib.EINVAL
        assert b"KCCOT_SMOOTH_CAUSAL_T" in lib.kccot_last_error()
        assert lib.kccot_smooth_bwd_f32(one, one, one, 2, 8, 9, 8, 1, 5.0, 3, flags, one, one, big, None) == _lib.EINVAL
        assert b"KCCOT_SMOOTH_CAUSAL_T" in lib.kccot_last_error()
        assert lib.kccot_smooth_bwd_sharded_f32(one, one, one, one, 2, 8, 9, 8, 1, 5.0, 3, flags | _lib.SMOOTH_EXTERNAL_STATS,
                                                one, one, big, None) == _lib.EINVAL
        assert b"KCCOT_SMOOTH_CAUSAL_T" in lib.kccot_last_error()
    # radius >= T is fine under the flag (no REFLECT padding), so the call gets as far as the workspace check
    assert lib.kccot_smooth_fwd_f32(one, 2, 8, 3, 8, 1, 5.0, 3, Cz | T, one, one, one, 16, None) == _lib.EWORKSPACE
    assert lib.kccot_smooth_fwd_f32(one, 2, 8, 3, 8, 1, 5.0, 8, Cz | T, one, one, one, big, None) == _lib.EUNSUPPORTED   # radius > 7
