/* kccot_smooth_causal3.h -- C ABI of the causal 3-D kernel smoothing of libkccot.so: past-only in time, symmetric in space.
 * An EXTENSION, NOT reference behaviour: the reference's 3-D smoothing (gaussian_convolution3D, KCCOT_SMOOTH_T|H|W in
 * kccot.h) uses the symmetric stencil along T as well, so frame t of the smoothed video contains frames t+1 .. t+r, and
 * kccot.h refuses KCCOT_SMOOTH_CAUSAL_T together with H or W.  These entry points are outside that header's versioned
 * surface (KCCOT_VERSION).  Strict C99.  Error codes, kccot_last_error(), kccot_stream_t and the KCCOT_SMOOTH_* protocol
 * flags are those of kccot.h; every call is asynchronous on `stream`, allocates nothing, never synchronises the host and
 * can be captured in a hipGraph.  All tensors are dense float32 [B,H,T,W,C] in device memory.
 *
 * Definition, with radius r (0 <= r <= 7), w_d = exp(-d^2 / (2 sigma^2)) and x the input:
 *   T, causal:      Z_t = sum_{d=0}^{min(r,t)} w_d,   a[t] = ( sum_{d=0}^{min(r,t)} w_d * x[t-d] ) * (1 / Z_t)
 *                   -- the formula of KCCOT_SMOOTH_CAUSAL_T: no padding, a[0] = x[0], any r is valid, r >= T included;
 *   W, then H:      the normalised (2r+1)-tap Gaussian with REFLECT borders of the symmetric 3-D call (needs r < H, r < W);
 *   normalisation:  out = s / max(s) over the WHOLE tensor: the arg-max element is exactly 1.0, a constant input gives ones.
 * Stage order T, W, H; every sum is fp32 fma in ascending tap index (T: ascending d), the 1 / Z_t multiply follows the T sum.
 * Backward: the adjoint of all of it, the arg-max path included (tied maxima share the correction, as in every smoothing
 * call): H^T and W^T with the border-folded weights, then (T^T y)[t'] = sum_{d=0}^{r, t'+d<T} (w_d / Z_{t'+d}) y[t'+d].
 *
 * flags carries ONLY the protocol bits of kccot.h, with their meaning and exclusivity rules there:
 *   KCCOT_SMOOTH_NO_DIVIDE, KCCOT_SMOOTH_EXTERNAL_MAX               (forward)
 *   KCCOT_SMOOTH_STATS_ONLY, KCCOT_SMOOTH_EXTERNAL_STATS            (kccot_smooth_causal3_bwd_sharded_f32: exactly one)
 * The axes are fixed: an axis bit (KCCOT_SMOOTH_T / _H / _W), KCCOT_SMOOTH_CAUSAL_T or any other bit returns KCCOT_EINVAL,
 * kccot_last_error() names the entry point, and nothing is launched.
 * Every argument check comes before any launch: KCCOT_EINVAL for a NULL pointer, a dimension < 1, sigma <= 0, radius >= H or
 * radius >= W, in == out, EXTERNAL_MAX with NO_DIVIDE, STATS_ONLY with EXTERNAL_STATS; KCCOT_EUNSUPPORTED for radius > 7;
 * KCCOT_EWORKSPACE for ws_bytes < kccot_smooth_workspace_bytes(B, H, T, W, C) (the query of kccot.h, unchanged).
 * Dispatch (options of kccot.h): radius 3 / 4 with C = 1 or 3 where option smooth_fused3 selects it: one fused walk each way
 * (radius 3 only for the adjoint); otherwise a chain of per-axis stages, for every radius, shape and alignment.  Where the
 * folded backward (option smooth_bwd_fold) would need more tie records than the workspace holds, the two-pass form runs.
 */
#ifndef KCCOT_SMOOTH_CAUSAL3_H
#define KCCOT_SMOOTH_CAUSAL3_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Parameters as kccot_smooth_fwd_f32: max_inout is one device float, written with the tensor maximum (READ under
 * KCCOT_SMOOTH_EXTERNAL_MAX); KCCOT_SMOOTH_NO_DIVIDE leaves `out` un-normalised and writes the local maximum. */
int kccot_smooth_causal3_fwd_f32(const float* in, int B, int H, int T, int W, int C, float sigma, int radius, unsigned flags,
                                 float* out, float* max_inout, void* ws, size_t ws_bytes, kccot_stream_t stream);
/* Parameters as kccot_smooth_bwd_f32: `out` and `max_in` are the forward's normalised output and maximum. */
int kccot_smooth_causal3_bwd_f32(const float* gout, const float* out, const float* max_in, int B, int H, int T, int W, int C,
                                 float sigma, int radius, unsigned flags, float* din, void* ws, size_t ws_bytes,
                                 kccot_stream_t stream);
/* Parameters as kccot_smooth_bwd_sharded_f32: stats_inout = {sum(gout * out), number of elements with out == 1}, written
 * under KCCOT_SMOOTH_STATS_ONLY (din is not touched, may be NULL), read under KCCOT_SMOOTH_EXTERNAL_STATS. */
int kccot_smooth_causal3_bwd_sharded_f32(const float* gout, const float* out, const float* max_in, float* stats_inout, int B,
                                         int H, int T, int W, int C, float sigma, int radius, unsigned flags, float* din,
                                         void* ws, size_t ws_bytes, kccot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_SMOOTH_CAUSAL3_H */
