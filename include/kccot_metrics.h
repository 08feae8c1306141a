/* kccot_metrics.h -- C ABI of the per-frame sample-quality metrics of libkccot.so: SSIM (with its adjoint with respect to the
 * generated video) and the mean squared error behind PSNR.  An EXTENSION, NOT reference behaviour: the reference publishes no
 * sample-quality figure.  These entry points are outside the versioned surface of kccot.h (KCCOT_VERSION).  Strict C99.  Error
 * codes, kccot_last_error() and kccot_stream_t are those of kccot.h; every call is asynchronous on `stream`, allocates nothing,
 * never synchronises the host and can be captured in a hipGraph.  x (real) and y (fake) are dense float32 [B,H,T,W,C] in
 * device memory; 4-byte alignment is enough.
 *
 * Definition (Wang et al. 2004 with a Gaussian window, VALID borders; scikit-image's structural_similarity with
 * gaussian_weights=True, use_sample_covariance=False and a mean over the border-cropped map, on this library's fp32 taps).
 * With r = radius, L = data_range and the taps w_0..w_2r of kccot_smooth_fwd_f32 (e_d = exp(-d^2 / (2 sigma^2)), d = -r..r, in
 * fp32, divided by their fp32 sum), for every frame (b,t) and channel c, at the map positions i in [0, H-2r), j in [0, W-2r):
 *     (G v)[i,j] = sum_a sum_b w_a w_b v[i+a, j+b]        a, b = 0..2r      (separable: W then H, fp32 fma)
 *     mx = G x,  my = G y,  sxx = G(x^2) - mx^2,  syy = G(y^2) - my^2,  sxy = G(xy) - mx my
 *     C1 = (0.01 L)^2,  C2 = (0.03 L)^2
 *     A1 = 2 mx my + C1,  A2 = 2 sxy + C2,  B1 = mx^2 + my^2 + C1,  B2 = sxx + syy + C2
 *     S  = A1 A2 / (B1 B2)
 *     ssim[b,t] = mean of S over i, j, c
 *     mse[b,t]  = mean of (x - y)^2 over h, w, c          (the difference in fp32, its square and the sum in fp64)
 * PSNR is the caller's 10 log10(L^2 / mse); x == y gives mse == 0 exactly.  Both means are fp64 sums: one partial per
 * workgroup, combined per frame in a fixed order by a second launch, rounded to fp32 at the end; no float atomics: two
 * identical calls give identical bits.
 *
 * Adjoint with respect to y for an upstream g[b,t].  With u = g[b,t] / ((H-2r)(W-2r)C) at every map position of the frame:
 *     alpha = -S / B2                                                          (dS / d G(y^2))
 *     beta  = 2 A1 / (B1 B2)                                                   (dS / d G(xy))
 *     gamma = 2 mx A2 / (B1 B2) - 2 my S / B1 - beta mx - 2 alpha my           (dS / d my in total)
 *     dy    = G^T(u gamma) + 2 y G^T(u alpha) + x G^T(u beta)
 *     (G^T m)[p,q] = sum_a sum_b w_a w_b m[p-a, q-b] over the terms inside the map.
 * Nothing is kept from the forward: the backward recomputes the moments from x and y.  mse has no adjoint here.
 *
 * Every argument check comes before any launch: KCCOT_EINVAL for a NULL tensor or result (mse_out alone may be NULL), a
 * dimension < 1, a sigma or data_range that is not > 0 (NaN included), a radius outside 0..7, 2 radius >= H or >= W, dy
 * overlapping x or y; KCCOT_EUNSUPPORTED only for a tensor too large to index (B*T, W*C or the workgroup count above 2^31 - 1);
 * KCCOT_EWORKSPACE for a NULL workspace or ws_bytes < kccot_ssim_workspace_bytes(B, H, T, W, C).
 */
#ifndef KCCOT_METRICS_H
#define KCCOT_METRICS_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for both entry points below at any radius (0 for a dimension < 1).  Nothing in it is tensor-sized: two
 * doubles per workgroup of the forward; the backward is one fused launch and keeps nothing there. */
size_t kccot_ssim_workspace_bytes(int B, int H, int T, int W, int C);

/* ssim_out [B*T] and, unless NULL, mse_out [B*T] of x (real) against y (fake). */
int kccot_ssim_fwd_f32(const float* x, const float* y, int B, int H, int T, int W, int C, float sigma, int radius,
                       float data_range, float* ssim_out, float* mse_out, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* dy [B,H,T,W,C] = d (sum_bt g[b,t] ssim[b,t]) / d y from g [B*T]. */
int kccot_ssim_bwd_f32(const float* g, const float* x, const float* y, int B, int H, int T, int W, int C, float sigma,
                       int radius, float data_range, float* dy, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* The tiling kccot_ssim_fwd_f32 (backward = 0) or kccot_ssim_bwd_f32 (backward != 0) would launch at this shape and radius: a
 * pure host function (no device call, no GPU needed) that runs the very planner of the launch, for tests and tools that must
 * know which tiling a case reaches.  The kernel is ssim_walk<radius, backward>.  Applies the argument checks of those entry
 * points that concern these arguments, with the same codes (KCCOT_EINVAL also for out == NULL).  out receives
 * KCCOT_SSIM_PLAN_INTS ints:
 *   [0] [1] [2]  wt, ct: the columns (of the map forward, of dy backward) and the channels of a tile; hs: the rows of a segment
 *   [3]          nt: the threads of a workgroup
 *   [4] [5] [6]  ntw, ntc, nseg: column tiles, channel tiles, segments along H
 *   [7]          the grid = B * T * nseg * ntw * ntc workgroups */
#define KCCOT_SSIM_PLAN_INTS 8
int kccot_ssim_plan(int B, int H, int T, int W, int C, int radius, int backward, int* out);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_METRICS_H */
