/* kccot_smooth_aniso.h -- C ABI of the ANISOTROPIC 3-D kernel smoothing of libkccot.so: one bandwidth and radius along T, another
 * along H and W.  An EXTENSION, NOT reference behaviour: the reference smooths all three axes with one sigma and one radius.
 * These entry points are outside the versioned surface of kccot.h (KCCOT_VERSION).  Strict C99.  Error codes,
 * kccot_last_error(), kccot_stream_t and the KCCOT_SMOOTH_* flags are those of kccot.h; every call is asynchronous on `stream`,
 * allocates nothing, never synchronises the host and can be captured in a hipGraph.  All tensors are dense float32 [B,H,T,W,C]
 * in device memory; 4-byte alignment is enough.
 *
 * Definition.  For a video x:
 *     s   = A_h(sigma_s, radius_s) A_w(sigma_s, radius_s) A_t(sigma_t, radius_t) x
 *     m   = max s over the whole tensor
 *     out = s / m
 *   A_w, A_h: the symmetric Gaussian stencil with REFLECT borders, w_d = e_d / sum_k e_k, d = -r..r,
 *       e_d = exp(-d^2 / (2 sigma^2)) (fp32 taps, evaluated as kccot_smooth_fwd_f32 evaluates them);
 *   A_t: the same symmetric REFLECT stencil with (sigma_t, radius_t), or, with KCCOT_SMOOTH_CAUSAL_T, the past-only stencil
 *       of kccot.h: row t uses v_{t,d} = e_d / Z_t, d = 0..min(radius_t, t), Z_t = e_0 + .. + e_min(radius_t,t); no padding,
 *       s[0] = x[0] along T;
 *   a radius of 0 makes that axis group the identity: radius_t = 0 means no T stencil, radius_s = 0 no H / W stencil.
 * The arg-max element of out is exactly 1.0f: the value that is divided and the value whose maximum is taken are the same
 * stored float.
 *
 * Backward.  With the upstream gradient g and n_ties = #(out == 1):
 *     u    = g / m - [out == 1] * (sum g*out) / (m * n_ties)              (the adjoint of the max-normalisation)
 *     din  = A_t^T A_w^T A_h^T u
 *     dsigma_t = sum_e u * (A_h A_w A'_t x)
 *     dsigma_s = sum_e u * ((A_h A'_w + A'_h A_w) A_t x)
 *   A' = the stencil with the derivative taps of kccot_smooth_sigma.h, from the sigma of that axis:
 *       symmetric  w'_d = w_d (d^2 - mu2) / sigma^3,  mu2 = sum_k w_k k^2;
 *       causal     v'_{t,d} = v_{t,d} (d^2 - mu2(t)) / sigma^3,  mu2(t) = sum_{k <= min(r,t)} v_{t,k} k^2;
 *   evaluated on the host in fp64 from the fp32 value of sigma and rounded to fp32.  A radius-0 axis group gives exactly 0
 *   for its dsigma.
 *   The adjoint of a REFLECT stencil of radius r on an axis of length L > r is a gather over q in [p-r, p+r] and [0, L) with
 *   the coefficient of u[q] in din[p]
 *       w[q-p] + [p >= 1 and p+q <= r] w[p+q] + [p <= L-2 and (L-1-p)+(L-1-q) <= r] w[2(L-1)-p-q];
 *   the adjoint of the causal stencil is din[p] = sum_{d = 0..r, p+d < T} v_{p+d,d} u[p+d].
 *   The stencil sums are fp32 fma; the sums over the elements of dsigma are fp64 (per-workgroup partials, combined by one
 *   workgroup in a fixed order, no float atomics): two identical calls give identical bits.
 *
 * flags.  The axes are fixed (T, H and W).  Accepted: KCCOT_SMOOTH_CAUSAL_T in every entry point; on the forward
 * KCCOT_SMOOTH_NO_DIVIDE (out stays s, max_inout receives the local maximum) or KCCOT_SMOOTH_EXTERNAL_MAX (max_inout is READ:
 * the batch-sharded caller has all-reduced the local maxima); on the sharded backward exactly one of KCCOT_SMOOTH_STATS_ONLY
 * (writes {sum g*out, n_ties} of this shard to stats_inout, din is not touched and may be NULL) and
 * KCCOT_SMOOTH_EXTERNAL_STATS (reads the global sums from stats_inout, writes din).  Any other bit -- an axis bit included --
 * returns KCCOT_EINVAL and kccot_last_error() names the flag.  A shard's out is bit-equal to its part of the one-call result.
 * The two sums are taken per sample and added over the samples in fp32 in sample order: shards of one sample each whose sums
 * are re-added in sample order (two shards: in either order) reproduce the one-call sums, and so din, bit for bit; any other
 * split agrees to the rounding of one fp32 sum.
 *
 * Every argument check comes before any launch: KCCOT_EINVAL for a refused flag, a NULL tensor / max / stats / result pointer,
 * a dimension < 1, a sigma that is not > 0 (NaN included), a radius outside 0..7, in == out on the forward,
 * radius_s >= H or >= W, radius_t >= T unless KCCOT_SMOOTH_CAUSAL_T (which takes any radius_t in 0..7); KCCOT_EWORKSPACE for a
 * NULL workspace or ws_bytes < kccot_smooth_aniso_workspace_bytes(B, H, T, W, C); KCCOT_EUNSUPPORTED only for a tensor too
 * large to index (T*W*C or B*H*T*W*C / 256 above 2^31 - 1).
 */
#ifndef KCCOT_SMOOTH_ANISO_H
#define KCCOT_SMOOTH_ANISO_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace for every entry point below, any radii and any flags at this shape (0 for a dimension < 1).  Nothing in
 * it is tensor-sized: one slot per workgroup of the largest grid any tiling launches, and the partial sums of the
 * normalisation's adjoint (one float per 1024 elements of a sample, one per sample). */
size_t kccot_smooth_aniso_workspace_bytes(int B, int H, int T, int W, int C);

/* out = the smoothing of in; max_inout: one device float, written (read with KCCOT_SMOOTH_EXTERNAL_MAX). */
int kccot_smooth_aniso_fwd_f32(const float* in, int B, int H, int T, int W, int C, float sigma_t, int radius_t, float sigma_s,
                               int radius_s, unsigned flags, float* out, float* max_inout, void* ws, size_t ws_bytes,
                               kccot_stream_t stream);

/* din = d loss / d in from gout = d loss / d out, the forward's out and the maximum it divided by. */
int kccot_smooth_aniso_bwd_f32(const float* gout, const float* out, const float* max_in, int B, int H, int T, int W, int C,
                               float sigma_t, int radius_t, float sigma_s, int radius_s, unsigned flags, float* din, void* ws,
                               size_t ws_bytes, kccot_stream_t stream);

/* The backward of a batch-sharded caller in two calls: KCCOT_SMOOTH_STATS_ONLY, (all-reduce SUM of stats_inout[0..1]),
 * KCCOT_SMOOTH_EXTERNAL_STATS.  max_in is the GLOBAL maximum. */
int kccot_smooth_aniso_bwd_sharded_f32(const float* gout, const float* out, const float* max_in, float* stats_inout, int B,
                                       int H, int T, int W, int C, float sigma_t, int radius_t, float sigma_s, int radius_s,
                                       unsigned flags, float* din, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* dsigma_out: two device floats {dsigma_t, dsigma_s}.  in: the forward's input.  stats_in = NULL: the two sums of u are taken
 * over this call's tensor; stats_in = {sum gout*out, n_ties} of the GLOBAL batch: the results are this shard's partials, the
 * caller adds the shards' partials up. */
int kccot_smooth_aniso_dsigma_f32(const float* in, const float* gout, const float* out, const float* max_in,
                                  const float* stats_in, int B, int H, int T, int W, int C, float sigma_t, int radius_t,
                                  float sigma_s, int radius_s, unsigned flags, float* dsigma_out, void* ws, size_t ws_bytes,
                                  kccot_stream_t stream);

/* The tiling an entry point above would launch at this shape, radii and flags: a pure host function (no device call, no GPU
 * needed) that runs the very planner of the launch, for tests and tools that must know which instantiation of the tile kernel a
 * case reaches.  job: 0 the forward, 1 the adjoint (either backward entry point), 2 dsigma; any other value is KCCOT_EINVAL.
 * Applies the argument checks of that job's entry points that concern these arguments, with the same codes (KCCOT_EINVAL also for
 * out == NULL); of flags only KCCOT_SMOOTH_CAUSAL_T changes the tiling.  out receives KCCOT_SMOOTH_ANISO_PLAN_INTS ints:
 *   [0]        1 when the call launches the tile kernel; 0 when it does not (job 2 with both radii 0: both results are exactly
 *              0) -- every other entry is then 0
 *   [1] [2] [3]  the instantiation aniso_tile<RS, NI, JOB>: RS = radius_s, NI = owned positions per thread, JOB = job
 *   [4..7]     the tile extents tt, wt, ct along T, W, C and the segment hs along H
 *   [8..11]    the piece counts ntt, ntw, ntc, nseg
 *   [12]       the grid = B * nseg * ntt * ntw * ntc workgroups */
#define KCCOT_SMOOTH_ANISO_PLAN_INTS 13
int kccot_smooth_aniso_plan(int B, int H, int T, int W, int C, int radius_t, int radius_s, unsigned flags, int job, int* out);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_SMOOTH_ANISO_H */
