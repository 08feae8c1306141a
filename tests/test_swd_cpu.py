"""CPU-side checks of the sliced Wasserstein distance (include/kccot_swd.h; not reference behaviour): the oracle of the GPU tests
(tests/swd_oracle.py) against the published Philox known answers, its prefix property, the moments of its directions, two closed
forms and autograd; the condition under which the GPU tests may compare with the oracle's own sort; the header against the
ctypes table and as strict C99; the argument rules that are decided before any launch (pointers that are never dereferenced);
the workspace and plan queries; and the Python path's refusals."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import swd_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kccot_swd_bwd_f32", "kccot_swd_directions_f32", "kccot_swd_fwd_f32", "kccot_swd_plan", "kccot_swd_workspace_bytes"]


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(counter, key, out):
    assert " ".join("%08x" % int(v) for v in so.philox4x32_10(counter, key)) == out


def test_direction_p_depends_on_neither_p_count_nor_k():
    full = so.directions(11, 1030, 0, 9)
    assert np.array_equal(so.directions(11, 517, 0, 9), full[:, :517])          # 517 % 4 != 0: a truncated last group
    assert np.array_equal(so.directions(11, 1030, 3, 4), full[3:7])
    assert np.array_equal(so.directions(11, 1, 8, 1), full[8:, :1])
    assert not np.array_equal(so.directions(12, 1030, 0, 9), full) and not np.array_equal(full[0], full[1])
    # the key is (seed & 0xffffffff, seed >> 32): the high word matters
    assert not np.array_equal(so.directions(11 + (1 << 32), 64, 0, 2), full[:2, :64])


def test_direction_moments_over_64_x_4096_samples():
    z = so.directions(7, 4096, 0, 64).ravel()
    n = z.size
    mean, std, m4 = float(z.mean()), float(z.std()), float((z ** 4).mean())
    print("mean %.4f  std %.4f  fourth moment %.3f over %d samples" % (mean, std, m4, n))
    # four standard errors of each estimator for N(0,1): 1 / sqrt(n), 1 / sqrt(2 n), sqrt((105 - 9) / n)
    assert abs(mean) <= 4 / np.sqrt(n) and abs(std - 1) <= 4 / np.sqrt(2 * n) and abs(m4 - 3) <= 4 * np.sqrt(96.0 / n)
    assert np.isfinite(z).all() and np.abs(z).max() <= np.sqrt(-2 * np.log(2.0 ** -24))


@pytest.mark.parametrize("B,P", [(1, 3), (5, 4), (16, 7)])
def test_k_equal_1_is_the_sorted_one_dimensional_squared_difference(B, P):
    real, fake, seed = so.make("noise", B, 1, 5)
    d = np.sort(real[:, 0].astype(np.float64)) - np.sort(fake[:, 0].astype(np.float64))
    assert np.abs(np.abs(so.unit_directions(seed, 1, P)) - 1).max() <= 1e-15          # theta^ = +-1
    assert abs(so.sw2(real, fake, seed, P) - float((d * d).mean())) <= 1e-15


@pytest.mark.parametrize("B,K,P,c", [(6, 40, 5, 0.25), (9, 7, 3, -1.5)])
def test_a_constant_shift_has_the_closed_form(B, K, P, c):
    real = so.make("noise", B, K, 2)[0].astype(np.float64)
    th = so.unit_directions(9, K, P)
    want = c * c * float((th.sum(1) ** 2).mean())
    assert abs(so.sw2(real, real + c, 9, P) - want) <= 1e-12 * max(1.0, want)


@pytest.mark.parametrize("kind", ["noise", "ties"])
@pytest.mark.parametrize("B,K,P", [(1, 7, 3), (8, 40, 5), (13, 9, 6)])
def test_closed_form_gradients_equal_autograd_of_the_oracles_value(B, K, P, kind):
    real, fake, seed = so.make(kind, B, K, 1)
    th = torch.from_numpy(so.unit_directions(seed, K, P))
    rv, fv = torch.from_numpy(real).double().requires_grad_(True), torch.from_numpy(fake).double().requires_grad_(True)
    v = so.sw2_torch(rv, fv, th)
    assert abs(float(v.detach()) - so.sw2(real, fake, seed, P)) <= 1e-15
    (1.5 * v).backward()
    dr, df = so.gradients(real, fake, seed, P, 1.5)
    assert np.abs(dr - rv.grad.numpy()).max() <= 1e-14 and np.abs(df - fv.grad.numpy()).max() <= 1e-14
    # at the oracle's own matching, given explicitly: the same
    a, b, _ = so.projections(real, fake, seed, P)
    dr2, df2 = so.gradients(real, fake, seed, P, 1.5, np.stack((so.stable_order(a), so.stable_order(b))))
    assert np.array_equal(dr, dr2) and np.array_equal(df, df2)


def test_ties_maker_ties_inside_and_across_the_batches():
    real, fake, _ = so.make("ties", 7, 12, 1)
    assert np.array_equal(real[1], real[2]) and np.array_equal(fake[1], fake[2])
    assert np.array_equal(fake[::3], real[::3]) and not np.array_equal(fake[1], real[1])
    assert np.array_equal(real * 8, np.round(real * 8))


@pytest.mark.parametrize("B,K,P,s", so.GAPPED)
def test_cases_compared_with_the_oracles_own_sort_have_gaps(B, K, P, s):
    real, fake, seed = so.make("noise", B, K, s)
    gap = so.min_gap(real, fake, seed, P)
    print("(%d,%d,%d) seed %d: smallest adjacent gap %.2e of the range" % (B, K, P, s, gap))
    assert gap >= so.MIN_GAP


# ---- the header ----------------------------------------------------------------------------------------------------------------
def _decls(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return dict((m.group(2), (m.group(1), m.group(3)))
                for m in re.finditer(r"\b(int|size_t)\s+(kccot_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text))


def test_header_and_ctypes_table_agree_and_stay_outside_the_versioned_surface():
    from kccotgan_amd import _lib
    decls = _decls("kccot_swd.h")
    assert sorted(decls) == NAMES and sorted(_lib.SWD_SIGNATURES) == NAMES
    ctype = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64,
             "unsigned": ctypes.c_uint, "uint64_t": ctypes.c_uint64}
    for name, (ret, args) in decls.items():
        want = [ctypes.c_void_p if ("*" in a or "kccot_stream_t" in a) else ctype[a.split()[0]] for a in args.split(",")]
        res, argtypes = _lib.SWD_SIGNATURES[name]
        assert res is ctype[ret] and argtypes == want, name
        fn = getattr(_lib.lib, name)
        assert fn.restype is ctype[ret] and list(fn.argtypes) == want
    assert not set(NAMES) & set(_decls("kccot.h")) and not set(NAMES) & set(_lib.SIGNATURES)
    text = open(os.path.join(ROOT, "include", "kccot_swd.h")).read()
    assert re.search(r"#define KCCOT_SWD_PLAN_INTS %d\b" % _lib.SWD_PLAN_INTS, text) and len(_lib._SWD_PLAN) == _lib.SWD_PLAN_INTS
    assert _lib.lib.kccot_version() == 301


def test_header_compiles_as_strict_c99(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text('#include "kccot_swd.h"\nint main(void) { return KCCOT_SWD_PLAN_INTS - 8 + KCCOT_SWD_MAX_B - 1024; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(probe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---- argument rules ------------------------------------------------------------------------------------------------------------
PTR = ctypes.c_void_p
X_, Y_, PR_, OR_, IN_, SW_, WS_, DX_, DY_, G_ = (1 << 22, 1 << 24, 1 << 26, 1 << 28, 1 << 30, 1 << 32, 1 << 34, 1 << 36, 1 << 38,
                                               1 << 40)                                          # never dereferenced
_p = lambda v: None if v is None else PTR(v)


def _fwd(**kw):
    from kccotgan_amd import _lib
    a = dict(real=X_, fake=Y_, B=3, K=7, P=5, proj=PR_, order=OR_, inv=IN_, out=SW_, ws=WS_, wsb=1 << 30)
    a.update(kw)
    return _lib.lib.kccot_swd_fwd_f32(_p(a["real"]), _p(a["fake"]), a["B"], a["K"], a["P"], 9, _p(a["proj"]), _p(a["order"]),
                                      _p(a["inv"]), _p(a["out"]), _p(a["ws"]), a["wsb"], None)


def _bwd(**kw):
    from kccotgan_amd import _lib
    a = dict(g=G_, proj=PR_, order=OR_, inv=IN_, B=3, K=7, P=5, dreal=DX_, dfake=DY_, ws=WS_, wsb=1 << 30)
    a.update(kw)
    return _lib.lib.kccot_swd_bwd_f32(_p(a["g"]), _p(a["proj"]), _p(a["order"]), _p(a["inv"]), a["B"], a["K"], a["P"], 9,
                                      _p(a["dreal"]), _p(a["dfake"]), _p(a["ws"]), a["wsb"], None)


def test_argument_rules_return_their_codes_before_any_launch():
    from kccotgan_amd import _lib
    err, lib = _lib.lib.kccot_last_error, _lib.lib
    # ---- forward (real, fake 84 bytes; proj, order 120; inv_norm 20; swd 4)
    for kw in ("real", "fake"):
        assert _fwd(**{kw: None}) == _lib.EINVAL and b"null input" in err(), kw
    for kw in ("proj", "order", "inv", "out"):
        assert _fwd(**{kw: None}) == _lib.EINVAL and b"null output" in err(), kw
    for kw in ("B", "K", "P"):
        for bad in (0, -2):
            assert _fwd(**{kw: bad}) == _lib.EINVAL and b"shape" in err(), (kw, bad)
    assert _fwd(B=1025) == _lib.EUNSUPPORTED and b"B=" in err()
    assert _fwd(P=65536) == _lib.EUNSUPPORTED and b"P=" in err()
    assert _fwd(K=(1 << 40) + 1) == _lib.EUNSUPPORTED and b"K=" in err()
    for kw in (dict(proj=X_), dict(proj=X_ + 80), dict(order=Y_ - 116), dict(inv=Y_ + 80), dict(out=X_ + 40), dict(order=PR_ + 116),
               dict(inv=PR_ - 16), dict(out=OR_ + 116), dict(out=IN_ + 16)):
        assert _fwd(**kw) == _lib.EINVAL and b"alias" in err(), kw
    need = lib.kccot_swd_workspace_bytes(3, 7, 5)
    assert need > 0 and need % 4 == 0
    assert _fwd(proj=X_ + 84, wsb=need - 1) == _lib.EWORKSPACE and b"workspace" in err()      # just clear of real
    assert _fwd(ws=None) == _lib.EWORKSPACE and _fwd(wsb=0) == _lib.EWORKSPACE
    assert _fwd(ws=WS_ + 8) == _lib.EINVAL and b"aligned" in err() and _bwd(ws=WS_ + 4) == _lib.EINVAL and b"aligned" in err()
    # ---- backward (dreal, dfake 84 bytes)
    for kw in ("g", "proj", "order", "inv"):
        assert _bwd(**{kw: None}) == _lib.EINVAL and b"null input" in err(), kw
    assert _bwd(dreal=None, dfake=None) == _lib.EINVAL and b"null output" in err()
    for kw in ("B", "K", "P"):
        for bad in (0, -1):
            assert _bwd(**{kw: bad}) == _lib.EINVAL and b"shape" in err(), (kw, bad)
    assert _bwd(B=1025) == _lib.EUNSUPPORTED and _bwd(P=65536) == _lib.EUNSUPPORTED and _bwd(K=(1 << 40) + 1) == _lib.EUNSUPPORTED
    for kw in (dict(dreal=G_), dict(dfake=G_ - 80), dict(dreal=PR_ + 116), dict(dfake=OR_ - 80), dict(dfake=IN_ + 16),
               dict(dfake=DX_ + 80), dict(dreal=DY_ - 80, dfake=DY_)):
        assert _bwd(**kw) == _lib.EINVAL and b"alias" in err(), kw
    assert _bwd(dfake=DX_ + 84, wsb=need - 1) == _lib.EWORKSPACE and b"workspace" in err()
    assert _bwd(dreal=None, ws=None) == _lib.EWORKSPACE and _bwd(dfake=None, wsb=0) == _lib.EWORKSPACE
    # ---- directions
    d = lib.kccot_swd_directions_f32
    assert d(1, 8, 0, 2, None, None) == _lib.EINVAL and b"null" in err()
    for K, p0, pc in ((0, 0, 1), (8, -1, 1), (8, 0, 0), (-3, 0, 2)):
        assert d(1, K, p0, pc, PTR(X_), None) == _lib.EINVAL and b"shape" in err(), (K, p0, pc)
    assert d(1, 8, 65535, 1, PTR(X_), None) == _lib.EUNSUPPORTED and d(1, 8, 0, 65536, PTR(X_), None) == _lib.EUNSUPPORTED
    assert d(1, (1 << 40) + 1, 0, 1, PTR(X_), None) == _lib.EUNSUPPORTED


def test_workspace_query_holds_the_partials_or_the_coefficients():
    from kccotgan_amd import _lib
    q = _lib.lib.kccot_swd_workspace_bytes
    assert q(0, 8, 4) == q(8, 0, 4) == q(8, 8, 0) == q(-1, 8, 4) == q(1025, 8, 4) == q(8, 8, 65536) == q(8, (1 << 40) + 1, 4) == 0
    up = lambda b: (b + 255) // 256 * 256
    for B, K, P in ((1, 1, 1), (3, 7, 5), (8, 1023, 16), (64, 122880, 128), (1024, 8, 2), (8, 3000, 200)):
        pl = _lib.swd_plan(B, K, P)
        fwd = up(pl["chunks"] * P * 2 * B * 4) + up(pl["chunks"] * P * 4) + up(P * 8)
        bwd = up(2 * B * ((P + 63) // 64 * 64) * 4)
        assert q(B, K, P) == max(fwd, bwd), (B, K, P)


def test_plan_query_reports_the_chunks_and_tiles_without_a_gpu():
    from kccotgan_amd import _lib
    pl = _lib.swd_plan(64, 122880, 128)                      # BASELINE configs[1], flattened
    assert pl == dict(kc=512, chunks=240, pt=64, rt=128, npt=2, nrt=1, np=64, kt=128)
    kc = _lib.swd_plan(8, 1, 1)["kc"]
    for K, chunks in ((1, 1), (kc, 1), (kc + 1, 2), (2 * kc, 2), (2 * kc + 3, 3)):
        pl = _lib.swd_plan(8, K, 4)
        assert pl["kc"] == kc and pl["chunks"] == chunks and pl["chunks"] == -(-K // pl["kc"])
    for B, np_, nrt in ((1, 1, 1), (2, 2, 1), (3, 4, 1), (64, 64, 1), (65, 128, 2), (70, 128, 2), (130, 256, 3), (1024, 1024, 16)):
        pl = _lib.swd_plan(B, 8, 2)
        assert (pl["np"], pl["nrt"]) == (np_, nrt), B
    assert [_lib.swd_plan(8, 8, P)["npt"] for P in (64, 65, 130, 65535)] == [1, 2, 3, 1024]
    big = _lib.swd_plan(8, 1 << 30, 4)                        # the chunk grows so that their number stays bounded
    assert big["chunks"] <= 1024 and big["kc"] % 64 == 0 and big["chunks"] == -(-(1 << 30) // big["kc"])
    out = (ctypes.c_int * _lib.SWD_PLAN_INTS)()
    lib, err = _lib.lib, _lib.lib.kccot_last_error
    assert lib.kccot_swd_plan(8, 8, 4, None) == _lib.EINVAL and b"null" in err()
    assert lib.kccot_swd_plan(0, 8, 4, out) == _lib.EINVAL and lib.kccot_swd_plan(8, 8, -1, out) == _lib.EINVAL
    assert lib.kccot_swd_plan(1025, 8, 4, out) == _lib.EUNSUPPORTED and lib.kccot_swd_plan(8, 8, 65536, out) == _lib.EUNSUPPORTED


# ---- Python ----------------------------------------------------------------------------------------------------------------------
def test_python_wrapper_refuses_bad_arguments_and_cpu_tensors():
    import inspect
    from kccotgan_amd import _lib, swd
    from kccotgan_amd.kernel_train import KCCOTTrainer
    sig = inspect.signature(swd.sliced_wasserstein2).parameters
    assert sig["n_projections"].default == 128 and sig["seed"].default == 0
    tsig = inspect.signature(KCCOTTrainer.swd).parameters
    assert list(tsig) == ["self", "real_data", "sigma", "n_projections", "seed"]
    assert (tsig["sigma"].default, tsig["n_projections"].default, tsig["seed"].default) == (None, 128, 0)
    assert "rank" in KCCOTTrainer.swd.__doc__
    x = torch.zeros((4, 3, 2))
    for bad in (dict(fake=torch.zeros((4, 6))), dict(fake=torch.zeros((3, 3, 2))), dict(real=torch.zeros(4), fake=torch.zeros(4)),
                dict(n_projections=0), dict(n_projections=65536), dict(n_projections=2.5), dict(seed=-1), dict(seed=1 << 64),
                dict(seed=0.5), dict(real=torch.zeros((0, 3)), fake=torch.zeros((0, 3)))):
        a = dict(real=x, fake=x, n_projections=4, seed=0)
        a.update(bad)
        with pytest.raises(ValueError, match="swd"):
            swd.sliced_wasserstein2(**a)
    with pytest.raises(NotImplementedError, match="B=1025"):
        swd.sliced_wasserstein2(torch.zeros((1025, 2)), torch.zeros((1025, 2)))
    with pytest.raises(_lib.KccotError):                      # no CPU path
        swd.sliced_wasserstein2(x, x, 4, 0)
    for bad in (dict(K=0), dict(p_begin=-1), dict(p_count=0), dict(p_begin=65535), dict(seed=-1)):
        a = dict(seed=0, K=8, p_begin=0, p_count=1)
        a.update(bad)
        with pytest.raises(ValueError, match="swd"):
            swd.directions(**a)
    with pytest.raises(_lib.KccotError):
        swd.directions(0, 8, 0, 1, device="cpu")
