"""KernelSmoothing held to float64 at the BASELINE shapes, forward and adjoint, every kernel family on its own.

The other smoothing tests meet fp64 at small shapes only (and the adjoint at 2e-4 of max|din|), compare the fused walks with
the per-axis chain, and plant arg-max ties into a synthetic forward output.  Here the fp64 reference (oracle/smoothing_torch.py,
pinned to the reference by tests/test_oracle_smoothing.py and tests/test_smoothing_golden.py) runs on the device next to the
kernels, on the whole tensor:

* forward: the whole output at the fixtures' tolerance (4e-6, temporal 1e-6), no rescaling; max(out) == 1 exactly, and the
  arg-max set {out == 1} equals the fp64 one, as does the tie count of the backward's statistics (STATS_ONLY);
* adjoint: din against smoothing_torch.smooth_bwd -- A^T (gout / max - corr [out == 1]), corr = sum(gout * out) / (max * n_ties),
  evaluated in fp64 from the kernel's own out and max -- at DIN_TOL of max|din_ref|.

Inputs are built so that the arg-max set is the same in fp32 and fp64 (checked: the largest non-tied fp64 value sits more than
1e-5 below the maximum):
  unique  one bright voxel on a k/255 background: the sparse fix-up with one tie;
  ties5   five identical voxels on a zero background, next to each other along W and C in one row of one sample (one
          workgroup's lines of the walks: more than TIE_PER_WG = 4 in one record, so the dense fallback);
  ties32  32 of them, four in that row and 28 spread: SMOOTH_MAX_TIES exactly, the sparse path at its limit;
  ties40  40 of them, five in that row: the dense fallback by count too;
  video   k/255 with saturated boxes larger than the stencil, one at the (0, 0, 0, 0) corner and one in the last frame (REFLECT
          folds taps onto them): the interior of every box ties -- and at sigma 0.03 every saturated voxel, thousands of ties.
The identical voxels sit 2R + 1 apart and more than R from every border, so their smoothed values are the same products
and tie exactly in either precision.  "video" is not run at sigma 0.3: there the neighbours of a box's interior fall short of
the maximum by ~w[2] = 2e-10 of it, below fp32's resolution and above fp64's, and the arg-max set is precision-dependent."""
import numpy as np
import pytest
import torch

ATOL_T, ATOL_3D = 1e-6, 4e-6            # tests/test_smoothing_golden.py
DIN_TOL = 1e-5                          # of max|din_ref|
SHAPES = {
    "cfg1": (64, 64, 30, 64, 1),
    "cfg2": (128, 64, 30, 64, 3),
    "cfg3": (256, 64, 30, 64, 3),
    "cfg4shard": (64, 128, 48, 128, 3),     # one rank's shard of configs[4] (512 samples over 8 ranks)
    "ragged3": (3, 37, 23, 45, 3),          # odd H and T, W * C = 135
    "ragged1": (5, 29, 31, 61, 1),          # W * C = 61
}
# name: (radius, flags = T 1 | H 2 | W 4, oracle axes); KernelSmoothing(6, 8): temporal radius 3, spatial radius 4
OPS = {"temporal": (3, 1, (2,)), "3d_r3": (3, 7, (2, 1, 3)), "3d_r4": (4, 7, (2, 1, 3)), "spatial": (4, 6, (1, 3))}
SIGMAS = (5.0, 1.3, 0.3, 0.03)          # annealing_sigma(5.0, step) reaches 0.03 after ~101 k steps
INPUTS = ("unique", "ties5", "ties32", "ties40", "video")
FAMILIES = {
    "default": {},
    "fused3=0": dict(smooth_fused3=0),
    "fused3=2": dict(smooth_fused3=2),
    "fold=0": dict(smooth_bwd_fold=0),
    "fold=1": dict(smooth_bwd_fold=1),
    "fold=2": dict(smooth_bwd_fold=2),
    "generic=1": dict(smooth_generic=1),
    "fused_tw=0": dict(smooth_fused_tw=0),
    "stream=0": dict(smooth_stream=0),
}
SPACING, MARGIN = 9, 5                  # 2R + 1 and R + 1 for the larger radius
FP64_ELEMS = 1 << 25                    # elements per fp64 slab of the adjoint reference


def _lattice(shape):
    """Positions along H, T, W that are SPACING apart and more than R from both borders."""
    return [list(range(MARGIN, n - MARGIN, SPACING)) for n in shape[1:4]]


def _voxels(shape, n_row, n_spread, rng):
    """n_row voxels in one row (sample 0, first lattice h and t; along W and C) + n_spread at random lattice points of the
    other samples."""
    B, H, T, W, C = shape
    lh, lt, lw = _lattice(shape)
    row = [(0, lh[0], lt[0], w, c) for w in lw for c in range(C)][:n_row]
    assert len(row) == n_row
    dims = (B - 1, len(lh), len(lt), len(lw), C)
    picks = rng.choice(int(np.prod(dims)), size=n_spread, replace=False)
    spread = [(1 + b, lh[i], lt[j], lw[k], c) for b, i, j, k, c in zip(*np.unravel_index(picks, dims))]
    return row + spread


def _input(kind, shape, seed):
    B, H, T, W, C = shape
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    if kind == "unique":
        x = torch.randint(0, 64, shape, device="cuda", generator=gen).float() / 255
        x[_voxels(shape, 0, 1, rng)[0]] = 1000.0
        return x
    if kind == "video":
        x = torch.randint(0, 200, shape, device="cuda", generator=gen).float() / 255
        x[0, :12, :12, :12, :] = 1.0                                        # the (0, 0, 0, 0) corner
        x[B - 1, H // 2 - 6:H // 2 + 6, T - 12:, W // 2 - 6:W // 2 + 6, :] = 1.0   # the last frame
        x[B // 2, H - 12:, T // 2 - 6:T // 2 + 6, W - 12:, :] = 1.0         # the far H and W borders
        return x
    n_row, n_spread = {"ties5": (5, 0), "ties32": (4, 28), "ties40": (5, 35)}[kind]
    x = torch.zeros(shape, device="cuda")
    for v in _voxels(shape, n_row, n_spread, rng):
        x[v] = 1.0
    return x


def _workspace(shape):
    from kccotgan_amd._lib import lib
    return torch.empty(int(lib.kccot_smooth_workspace_bytes(*shape)), dtype=torch.uint8, device="cuda")


def _fwd(x, sigma, radius, flags, mx=None):
    from kccotgan_amd._lib import lib, check, ptr, stream_of
    out = torch.empty_like(x)
    m = torch.empty(1, device="cuda") if mx is None else mx.clone()
    ws = _workspace(x.shape)
    check(lib.kccot_smooth_fwd_f32(ptr(x), *x.shape, sigma, radius, flags, ptr(out), ptr(m), ws.data_ptr(), ws.numel(),
                                   stream_of(x)), "smooth_fwd")
    return out, m


def _bwd(g, out, mx, sigma, radius, flags, stats=None):
    """One-call backward; with ``stats``: the sharded entry point, EXTERNAL_STATS (stats handed in) -- or STATS_ONLY when
    ``stats`` is the string "only" (returns the two sums)."""
    from kccotgan_amd import _lib
    from kccotgan_amd._lib import lib, check, ptr, stream_of
    ws = _workspace(out.shape)
    din = torch.empty_like(out)
    if stats is None:
        check(lib.kccot_smooth_bwd_f32(ptr(g), ptr(out), ptr(mx), *out.shape, sigma, radius, flags, ptr(din), ws.data_ptr(),
                                       ws.numel(), stream_of(out)), "smooth_bwd")
        return din
    only = isinstance(stats, str)
    st = torch.zeros(2, device="cuda") if only else stats
    check(lib.kccot_smooth_bwd_sharded_f32(ptr(g), ptr(out), ptr(mx), ptr(st), *out.shape, sigma, radius,
                                           flags | (_lib.SMOOTH_STATS_ONLY if only else _lib.SMOOTH_EXTERNAL_STATS), ptr(din),
                                           ws.data_ptr(), ws.numel(), stream_of(out)), "smooth_bwd_sharded")
    return st if only else din


def _slab(shape):
    return max(1, FP64_ELEMS // int(np.prod(shape[1:])))


def _reference(x, sigma, radius, axes):
    """fp64 forward of the whole tensor, its arg-max mask and the gap to the largest non-tied value."""
    from oracle import smoothing_torch as st
    ref = st.smooth(x.double(), sigma, radius, axes)
    ties = ref == 1
    gap = 1.0 - float(ref.masked_fill(ties, -1.0).max())
    return ref, ties, gap


def _cell(shape_name, op, sigma, kind, x, g, rows, fails, families=FAMILIES):
    """Every family on one (shape, operation, sigma, input): forward and adjoint against fp64."""
    from kccotgan_amd import _lib
    from oracle import smoothing_torch as st
    radius, flags, axes = OPS[op]
    atol = ATOL_T if op == "temporal" else ATOL_3D
    ref, ties, gap = _reference(x, sigma, radius, axes)
    n_ties = int(ties.sum())
    tag = "%-9s %-8s sigma=%-4g %-6s" % (shape_name, op, sigma, kind)
    assert gap > 1e-5, (tag, "input has a near-tie in fp64", gap)
    cached = None                        # (out, mx, din_ref, scale) of the last distinct forward
    for fam, opts in families.items():
        with _lib.options(**opts):
            out, mx = _fwd(x, sigma, radius, flags)
            din = _bwd(g, out, mx, sigma, radius, flags)
            stats = _bwd(g, out, mx, sigma, radius, flags, stats="only")
        torch.cuda.synchronize()
        fwd_err = float((out.double() - ref).abs().max())
        kmax = float(out.max())
        same_argmax = bool(torch.equal(out == 1, ties))
        k_ties = int(stats[1])
        if cached is None or not (torch.equal(cached[0], out) and torch.equal(cached[1], mx)):
            cached = None
            din_ref = st.smooth_bwd(g, out, mx, sigma, radius, axes, slab=_slab(out.shape))
            cached = (out, mx, din_ref, float(din_ref.abs().max()))
        din_err = float((din.double() - cached[2]).abs().max()) / cached[3]
        rows.append((din_err, "%s %-10s fwd %.2e  din %.2e  ties %d" % (tag, fam, fwd_err, din_err, n_ties)))
        bad = []
        if kmax != 1.0:
            bad.append("max(out) = %r" % kmax)
        if fwd_err > atol:
            bad.append("forward %.3e > %.0e" % (fwd_err, atol))
        if not same_argmax:
            bad.append("arg-max set: %d kernel, %d fp64" % (int((out == 1).sum()), n_ties))
        if k_ties != n_ties:
            bad.append("STATS_ONLY ties %d != %d" % (k_ties, n_ties))
        if not din_err <= DIN_TOL:
            bad.append("adjoint %.3e > %.0e" % (din_err, DIN_TOL))
        if bad:
            fails.append("%s %s: %s" % (tag, fam, "; ".join(bad)))
        del out, mx, din, stats
    del ref, ties, cached


def _report(rows, fails):
    for _, line in rows:
        print(line)
    worst = sorted(rows, reverse=True)[:3]
    print("worst adjoint cells:\n  " + "\n  ".join(line for _, line in worst))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("op", list(OPS))
@pytest.mark.parametrize("shape_name", list(SHAPES))
def test_smoothing_families_against_fp64(shape_name, op):
    """Forward and adjoint of every kernel family against fp64, at four sigmas and five inputs (module docstring); prints the
    worst error of every cell (-s)."""
    import kccotgan_amd  # noqa: F401  (before the first CUDA call: kccotgan_amd/__init__.py)
    shape = SHAPES[shape_name]
    rows, fails = [], []
    g = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    for i, kind in enumerate(INPUTS):
        x = _input(kind, shape, 100 + i)
        for sigma in SIGMAS:
            if kind == "video" and sigma == 0.3:
                continue                 # precision-dependent arg-max set (module docstring)
            _cell(shape_name, op, sigma, kind, x, g, rows, fails)
        del x
    del g
    torch.cuda.empty_cache()
    _report(rows, fails)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["temporal", "3d_r3", "3d_r4"])
def test_emulated_eight_rank_sharded_smoothing_at_configs3(op):
    """The data-parallel protocol of _SmoothSharded at its real size, eight "ranks" in one process: configs[3] cut into eight
    slabs of 32 samples; forward per slab with NO_DIVIDE, the maximum of the eight maxima taken on the host, then per slab with
    EXTERNAL_MAX; backward per slab with STATS_ONLY, the sums added on the host, then per slab with EXTERNAL_STATS.  The slabs
    (11.8 M elements) take other kernels than the whole batch (94 M): the stitched forward must still equal the one-call
    forward bit for bit, and the stitched adjoint meet the fp64 bound."""
    from kccotgan_amd import _lib       # (before the first CUDA call: kccotgan_amd/__init__.py)
    from oracle import smoothing_torch as st
    shape = SHAPES["cfg3"]
    radius, flags, axes = OPS[op]
    g = torch.randn(shape, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    rows, fails = [], []
    for kind, sigma in (("video", 0.03), ("ties40", 1.3), ("unique", 5.0)):
        x = _input(kind, shape, 200 + len(kind))
        one, m1 = _fwd(x, sigma, radius, flags)
        slabs = [slice(32 * r, 32 * (r + 1)) for r in range(8)]
        maxima = [float(_fwd(x[s], sigma, radius, flags | _lib.SMOOTH_NO_DIVIDE)[1]) for s in slabs]
        mx = torch.tensor([max(maxima)], device="cuda")
        out = torch.cat([_fwd(x[s], sigma, radius, flags | _lib.SMOOTH_EXTERNAL_MAX, mx)[0] for s in slabs])
        torch.cuda.synchronize()
        assert float(mx) == float(m1), (op, kind)
        assert torch.equal(out, one), (op, kind, float((out - one).abs().max()))
        del one
        parts = [_bwd(g[s], out[s], mx, sigma, radius, flags, stats="only").double().cpu() for s in slabs]
        stats = torch.stack(parts).sum(0).float().cuda()
        din = torch.cat([_bwd(g[s], out[s], mx, sigma, radius, flags, stats=stats) for s in slabs])
        torch.cuda.synchronize()
        whole = st.maxnorm_stats(g, out)
        assert int(stats[1]) == whole[1], (op, kind, int(stats[1]), whole[1])
        ref = st.smooth_bwd(g, out, mx, sigma, radius, axes, stats=whole, slab=_slab(shape))
        err = float((din.double() - ref).abs().max()) / float(ref.abs().max())
        rows.append((err, "cfg3 x 8  %-8s sigma=%-4g %-6s sharded    din %.2e  ties %d" % (op, sigma, kind, err, whole[1])))
        if not err <= DIN_TOL:
            fails.append("%s %s: sharded adjoint %.3e > %.0e" % (op, kind, err, DIN_TOL))
        del x, out, din, ref
    torch.cuda.empty_cache()
    _report(rows, fails)
