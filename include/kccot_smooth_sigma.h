/* kccot_smooth_sigma.h -- C ABI of the gradient of the kernel smoothing of libkccot.so with respect to its bandwidth sigma.
 * An EXTENSION, NOT reference behaviour: the reference treats sigma as a constant that a hand-set schedule anneals.  These
 * entry points are outside the versioned surface of kccot.h (KCCOT_VERSION).  Strict C99.  Error codes, kccot_last_error(),
 * kccot_stream_t and the KCCOT_SMOOTH_* flags are those of kccot.h; the call is asynchronous on `stream`, allocates nothing,
 * never synchronises the host and can be captured in a hipGraph.  All tensors are dense float32 [B,H,T,W,C] in device memory;
 * 4-byte alignment is enough.
 *
 * Definition.  s = A(sigma) x is the un-normalised smoothing (A = the product of the per-axis operators of the axes in
 * axes_flags), m = max s over the whole tensor, out = s / m.  With e_d = exp(-d^2 / (2 sigma^2)):
 *   symmetric axis (REFLECT borders, radius r):  w_d = e_d / sum_k e_k,  d = -r..r;
 *       w'_d = w_d (d^2 - mu2) / sigma^3,  mu2 = sum_k w_k k^2   (so sum_d w'_d = 0);  A'_a = the same stencil with w';
 *   causal T axis (KCCOT_SMOOTH_CAUSAL_T; no padding):  row t uses v_{t,d} = e_d / Z_t, d = 0..min(r,t);
 *       v'_{t,d} = v_{t,d} (d^2 - mu2(t)) / sigma^3,  mu2(t) = sum_{k <= min(r,t)} v_{t,k} k^2;
 *   ds/dsigma = sum_a ( prod_{b != a} A_b ) A'_a x;
 *   u = gout / m - [out == 1] * (sum gout*out) / (m * n_ties)        (the adjoint of the max-normalisation);
 *   dsigma = sum_e u[e] * (ds/dsigma)[e].
 * w' and v' are evaluated on the host in fp64 from the fp32 value of sigma and rounded to fp32; the sums over the stencils are
 * fp32 fma, the sum over the elements is fp64 (per-workgroup partials, combined by one workgroup in a fixed order, no float
 * atomics): two identical calls give identical bits.  radius = 0 (or no axis bit) gives exactly 0.
 *
 * axes_flags: any of KCCOT_SMOOTH_T | _H | _W, optionally with KCCOT_SMOOTH_CAUSAL_T (needs KCCOT_SMOOTH_T; here, unlike in
 * kccot.h, T|H|W|CAUSAL_T is accepted and means the causal 3-D form of kccot_smooth_causal3.h).  A protocol bit (NO_DIVIDE,
 * EXTERNAL_MAX, STATS_ONLY, EXTERNAL_STATS), CAUSAL_T without T or an unknown bit returns KCCOT_EINVAL and kccot_last_error()
 * names the flag.
 * Every argument check comes before any launch: KCCOT_EINVAL for a NULL tensor / max / result pointer, a dimension < 1,
 * sigma <= 0, radius outside 0..7, radius >= the length of a symmetric (REFLECT) axis; KCCOT_EWORKSPACE for a NULL workspace or
 * ws_bytes < kccot_smooth_dsigma_workspace_bytes(B, H, T, W, C); KCCOT_EUNSUPPORTED for a tensor too large to index.
 */
#ifndef KCCOT_SMOOTH_SIGMA_H
#define KCCOT_SMOOTH_SIGMA_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for any radius, any axes_flags and either value of stats_in at this shape (0 for a dimension < 1). */
size_t kccot_smooth_dsigma_workspace_bytes(int B, int H, int T, int W, int C);

/* in: the forward's input; out, max_in: its normalised output and the maximum it divided by (for a batch-sharded caller the
 * GLOBAL maximum); gout: the gradient arriving at out.  stats_in = NULL: the two sums of u are taken over this call's tensor
 * (the same two-pass form, and the same bits, as KCCOT_SMOOTH_STATS_ONLY).  stats_in = {sum gout*out, n_ties} of the GLOBAL
 * batch: the result is this shard's partial, the caller adds the shards' partials up.  dsigma_out: one device float. */
int kccot_smooth_dsigma_f32(const float* in, const float* gout, const float* out, const float* max_in, const float* stats_in,
                            int B, int H, int T, int W, int C, float sigma, int radius, unsigned axes_flags,
                            float* dsigma_out, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* The tiling kccot_smooth_dsigma_f32 would launch at this shape, radius and axes_flags: a pure host function (no device call,
 * no GPU needed) that runs the very planner of the launch, for tests and tools that must know which instantiation of the tile
 * kernel a case reaches.  Applies the argument checks of kccot_smooth_dsigma_f32 that concern these arguments, with the same
 * codes (KCCOT_EINVAL also for out == NULL).  out receives KCCOT_SMOOTH_DSIGMA_PLAN_INTS ints:
 *   [0]       1 when the call launches the tile kernel; 0 when it does not (radius 0, or no axis bit: the result is exactly
 *             0) -- every other entry is then 0
 *   [1] [2]   the instantiation dsigma_tile<R, NI>: R = radius, NI = owned positions per thread
 *   [3..6]    the tile extents tt, wt, ct along T, W, C and the segment hs along H
 *   [7..10]   the piece counts ntt, ntw, ntc, nseg
 *   [11]      the grid = B' * nseg * ntt * ntw * ntc workgroups
 *   [12..16]  B', H', T', W', C': the kernel's view of the shape, in which [3..11] are expressed: an axis that is not smoothed
 *             has been merged into its neighbour (W into C when W is not smoothed, B into H when H is not). */
#define KCCOT_SMOOTH_DSIGMA_PLAN_INTS 17
int kccot_smooth_dsigma_plan(int B, int H, int T, int W, int C, int radius, unsigned axes_flags, int* out);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_SMOOTH_SIGMA_H */
