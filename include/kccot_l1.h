/* kccot_l1.h -- C ABI of the adjoint of the L1 ground cost of libkccot.so (the forward is the flag KCCOT_COST_L1 of
 * kccot_pairwise_cost_f32 / kccot_pairwise_cost3_f32 in kccot.h).  An EXTENSION, NOT reference behaviour: the reference's
 * docstrings call its transport cost an L1 cost, its code computes the squared L2 distance, and that stays the default.  These
 * entry points are outside the versioned surface of kccot.h (KCCOT_VERSION).  Strict C99.  Error codes, kccot_last_error()
 * and kccot_stream_t are those of kccot.h; every call is asynchronous on `stream`, allocates nothing, never synchronises the
 * host and can be captured in a hipGraph.  All tensors are dense float32 in device memory; 4-byte alignment is enough.
 *
 * Definition.  With x [Bx,K], y [By,K] and the scaling coefficient sc,
 *     C[i,j] = sc * sum_k |x[i,k] - y[j,k]|      (+ the causal terms of kccot_pairwise_cost_f32, which do not depend on x, y)
 * and, for an upstream g [Bx,By], with sgn(0) = 0 (what differentiating |.| at a tie gives in torch):
 *     dx[i,k] = sc * sum_j g[i,j] sgn(x[i,k] - y[j,k])
 *     dy[j,k] = sc * sum_i g[i,j] sgn(y[j,k] - x[i,k])
 *     KCCOT_COST_SAME (x is y):  dx[i,k] = sc * sum_j (g[i,j] + g[j,i]) sgn(x[i,k] - x[j,k])
 *     loss form (g3 = [gxy, gxx, gyy] of C3 = [xy, xx, yy], kccot_pairwise_cost3_f32):
 *         dfake[j,k] = sc * sum_i ( gxy[i,j] sgn(fake[j,k] - real[i,k]) + (gyy[i,j] + gyy[j,i]) sgn(fake[j,k] - fake[i,k]) )
 * All four are out[r,k] = sc * sum_{c<N} W[r,c] sgn(a[r,k] - S[c,k]): a small launch writes the coefficient matrix W into the
 * workspace (the only thing kept there: nothing is tensor-sized), a second one walks the source rows S -- for the loss form
 * real then fake, in place -- once per group of eight target rows.  The sign is a pair of fp32 comparisons of the two values
 * (with gradual underflow the sign of the fp32 difference): a tie contributes exactly 0, whatever its coefficient.  The sum over c
 * runs in fp32 in the fixed order c = 0..N-1 per element, sc is applied once at the end, and there are no atomics: two identical
 * calls give identical bits.
 *
 * The feature gradients (dh, dM) do not depend on the ground cost: kccot_pairwise_cost_bwd_f32 with dx = dy = NULL and
 * kccot_pairwise_cost3_bwd_f32 with dfake = NULL give them.
 *
 * Every argument check comes before any launch: KCCOT_EINVAL for a NULL input, no output at all, a dimension < 1, flags other
 * than 0 or KCCOT_COST_SAME, KCCOT_COST_SAME without x == y, Bx == By and dy == NULL, an output overlapping an input or the
 * other output; KCCOT_EWORKSPACE for a NULL workspace or ws_bytes below the query; KCCOT_EUNSUPPORTED only for sizes that cannot
 * be indexed (more than 524280 target rows, more than 2^31 - 1 column tiles of 1024).  Any B >= 1 and any K >= 1.
 */
#ifndef KCCOT_L1_H
#define KCCOT_L1_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of workspace of kccot_l1_cost_bwd_f32: the two coefficient matrices (0 for a dimension < 1). */
size_t kccot_l1_cost_bwd_workspace_bytes(int Bx, int By);

/* dx [Bx,K] and / or dy [By,K] (either may be NULL, not both) from g [Bx,By].  flags: 0 or KCCOT_COST_SAME. */
int kccot_l1_cost_bwd_f32(const float* g, const float* x, const float* y, int Bx, int By, int64_t K, float sc, unsigned flags,
                          float* dx, float* dy, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* Bytes of workspace of kccot_l1_cost3_bwd_f32: the [2B, B] coefficient matrix (0 for B < 1). */
size_t kccot_l1_cost3_bwd_workspace_bytes(int B);

/* dfake [B,K] from g3 [3,B,B] (the loss form above; gxx is not read: the loss never differentiates w.r.t. real). */
int kccot_l1_cost3_bwd_f32(const float* g3, const float* real, const float* fake, int B, int64_t K, float sc, float* dfake,
                           void* ws, size_t ws_bytes, kccot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_L1_H */
