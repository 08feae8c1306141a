"""Known-answer tests pinning the KernelSmoothing oracle (oracle/smoothing_np.py) -- the
reference's data_utils.py cannot be imported here and has no fixtures, so
these KATs are derived from the cited reference lines.  CPU only."""
import numpy as np
import pytest
from scipy import ndimage

from oracle import smoothing_np as sm


def test_taps_sum_to_one_and_are_symmetric():     # data_utils.py:488-491
    for r, s in ((3, 5.0), (3, 0.7), (4, 2.0)):
        k = sm.gaussian_kernel1d(r, s)
        assert k.dtype == np.float32 and len(k) == 2 * r + 1
        assert abs(float(k.sum()) - 1) < 1e-6 and np.allclose(k, k[::-1])
    k3 = sm.gaussian_kernel3d(3, 5.0)
    assert k3.shape == (7, 7, 7) and abs(float(k3.sum()) - 1) < 1e-5
    k1 = sm.gaussian_kernel1d(3, 5.0)
    np.testing.assert_allclose(k3, np.einsum("a,b,c->abc", k1, k1, k1), rtol=2e-6)   # separable


def test_constant_video_gives_ones():              # smoothed == const, / max -> 1 (data_utils.py:520)
    v = np.full((2, 8, 9, 8, 1), 0.37, np.float32)
    np.testing.assert_allclose(sm.temporal_convolution(v, 5.0), 1.0, rtol=1e-6)
    np.testing.assert_allclose(sm.gaussian_convolution3D_separable(v, 5.0), 1.0, rtol=1e-6)


def test_reflect_border_does_not_repeat_the_edge():   # data_utils.py:512-513: tf.pad REFLECT
    v = np.zeros((1, 1, 8, 1, 1), np.float32)
    v[0, 0, :, 0, 0] = np.arange(8)
    w = sm.gaussian_kernel1d(3, 5.0)
    s = sm._conv_axis(v, w, 2)[0, 0, :, 0, 0]
    padded = np.array([3, 2, 1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4], np.float32)
    np.testing.assert_allclose(s, np.correlate(padded, w, mode="valid"), rtol=1e-6)
    np.testing.assert_allclose(s, ndimage.correlate1d(v[0, 0, :, 0, 0], w, mode="mirror"), rtol=1e-6)


@pytest.mark.parametrize("C", [1, 3])
def test_dense_3d_equals_separable_and_scipy(C):      # data_utils.py:552-582
    rng = np.random.default_rng(C)
    v = rng.random((2, 9, 8, 10, C), dtype=np.float32)
    dense = sm.gaussian_convolution3D(v, 2.0, normalise=False)
    sep = sm.gaussian_convolution3D_separable(v, 2.0, normalise=False)
    np.testing.assert_allclose(dense, sep, rtol=2e-5, atol=2e-6)
    k = sm.gaussian_kernel3d(3, 2.0)
    for b in range(2):
        for c in range(C):
            ref = ndimage.correlate(v[b, :, :, :, c].astype(np.float64), k.astype(np.float64), mode="mirror")
            np.testing.assert_allclose(dense[b, :, :, :, c], ref, rtol=2e-5, atol=2e-6)
    out = sm.gaussian_convolution3D(v, 2.0)
    assert abs(float(out.max()) - 1) < 1e-6


def test_sigma_schedule():                          # data_utils.py:584-586
    assert sm.annealing_sigma(5.0, 0) == 5.0
    assert abs(sm.annealing_sigma(5.0, 500) - 5.0 * 0.975) < 1e-12
    assert abs(sm.annealing_sigma(5.0, 250) - 5.0 * 0.975 ** 0.5) < 1e-12


def test_torch_flavour_matches_numpy():
    import torch
    from oracle import smoothing_torch as st
    v = np.random.default_rng(5).random((2, 9, 8, 10, 3), dtype=np.float32)
    np.testing.assert_allclose(st.smooth(torch.from_numpy(v), 2.0, 3, (2,)).numpy(),
                               sm.temporal_convolution(v, 2.0), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(st.smooth(torch.from_numpy(v), 5.0, 3, (2, 1, 3)).numpy(),
                               sm.gaussian_convolution3D_separable(v, 5.0), rtol=1e-5, atol=1e-6)


def test_torch_full_max_gradient_splits_evenly_over_ties():
    """The reference's reduce_max gradient goes in equal parts to every exact tie; smoothing_torch.smooth_bwd restates it as
    corr / n_ties.  Checked here on torch's own full-reduction max() rather than assumed, since the pinning below uses it."""
    import torch
    v = torch.tensor([0.5, 2.0, -1.0, 2.0, 1.0, 2.0], dtype=torch.float64, requires_grad=True)
    (g,) = torch.autograd.grad(v.max(), v)
    assert g.tolist() == [0.0, 1 / 3, 0.0, 1 / 3, 0.0, 1 / 3]
    (g,) = torch.autograd.grad(v[:3].max(), v)                 # one arg-max: all of it
    assert g.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0]


def _tie_video(ties, shape, radius, rng):
    """fp64 input whose smoothed maximum is tied exactly ``ties`` times (0 / 1: a unique maximum): identical bright voxels
    at least 2R + 1 apart and more than R from every border (their stencils neither overlap nor fold: a voxel R from the
    border would be counted twice by the border position and outweigh itself under a flat kernel), on a zero background;
    "blob": a saturated box larger than the stencil in a k/255 background, touching the (0, 0, 0) corner."""
    import torch
    B, H, T, W, C = shape
    v = np.zeros(shape)
    if ties == "blob":
        v[:] = rng.integers(0, 200, shape) / 255.0
        v[0, :2 * radius + 3, :2 * radius + 3, :2 * radius + 3, :] = 1.0
        return torch.from_numpy(v)
    s = 2 * radius + 1
    lattice = [(b, h, t, w, c) for b in range(B) for h in range(radius + 1, H - radius - 1, s)
               for t in range(radius + 1, T - radius - 1, s) for w in range(radius + 1, W - radius - 1, s) for c in range(C)]
    pick = rng.choice(len(lattice), size=max(ties, 1), replace=False)
    for i in pick:
        v[lattice[i]] = 1.0
    if ties == 0:
        v[lattice[pick[0]]] = 1.25
    return torch.from_numpy(v)


@pytest.mark.parametrize("axes", [(2,), (2, 1, 3), (1, 3)])
@pytest.mark.parametrize("ties", [0, 1, 3, 11, "blob"])
def test_adjoint_helper_equals_fp64_autograd(axes, ties):
    """smoothing_torch.smooth_bwd (A^T of the unnormalised smoothing, the normalisation's adjoint written out, the way the GPU
    tests evaluate it at full size) against plain fp64 autograd of smooth(...): 0, 1, 3 and 11 exact arg-max ties, and a
    saturated blob at sigma 0.03 (every saturated voxel ties) and 1.3 (the blob's interior ties), folded at the corner.
    ties = 0 means: the helper is handed an ``out`` with no element exactly 1 (what a kernel that misses its arg-max would
    produce) and must then equal the gradient with the maximum held constant."""
    import torch
    from oracle import smoothing_torch as st
    rng = np.random.default_rng(7 + len(axes) + (ties if isinstance(ties, int) else 40))
    shape, radius = (2, 19, 20, 21, 2), 3
    x = _tie_video(ties, shape, radius, rng)
    for sigma in ((0.03, 1.3) if ties == "blob" else (5.0, 0.3)):
        xd = x.clone().requires_grad_(True)
        s = st.smooth(xd, sigma, radius, axes, normalise=False)
        m = s.max()
        out = s / (m.detach() if ties == 0 else m)
        g = torch.from_numpy(rng.standard_normal(shape))
        (want,) = torch.autograd.grad(out, xd, g)
        out = out.detach()
        n = int((out == 1).sum())
        if ties == 0:
            out = torch.where(out == 1, torch.full_like(out, 1 - 1e-12), out)
            n = 0
        elif ties == "blob":
            assert n >= (1 if sigma > 1 else 3) * (3 ** len(axes)) * 2, n        # thousands at full size
        else:
            assert n == ties
        assert st.maxnorm_stats(g, out)[1] == n
        got = st.smooth_bwd(g, out, m.detach(), sigma, radius, axes)
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-12 * float(want.abs().max()),
                                   err_msg=str((axes, ties, sigma)))
        # slab by slab with the whole tensor's sums handed in: the same numbers (A^T does not couple samples)
        half = st.smooth_bwd(g[:1], out[:1], m.detach(), sigma, radius, axes, stats=st.maxnorm_stats(g, out))
        np.testing.assert_allclose(half.numpy(), got[:1].numpy(), rtol=0, atol=1e-14 * float(want.abs().max()))
        np.testing.assert_allclose(st.smooth_bwd(g, out, m.detach(), sigma, radius, axes, slab=1).numpy(), got.numpy(),
                                   rtol=0, atol=1e-14 * float(want.abs().max()))
        if n > 1:                            # the 1 / n_ties split is visible at this tolerance
            wrong = st.smooth_bwd(g, out, m.detach(), sigma, radius, axes, stats=(st.maxnorm_stats(g, out)[0], 1))
            assert float((wrong - want).abs().max()) > 1e-6 * float(want.abs().max())
