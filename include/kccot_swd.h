/* kccot_swd.h -- C ABI of the sliced Wasserstein distance (order 2, squared) between two batches of libkccot.so, with its adjoint
 * with respect to both batches.  An EXTENSION, NOT reference behaviour: the reference has no distance between the real and the
 * generated distribution that is free of learned features.  These entry points are outside the versioned surface of kccot.h
 * (KCCOT_VERSION).  Strict C99.  Error codes, kccot_last_error() and kccot_stream_t are those of kccot.h; every device call is
 * asynchronous on `stream`, allocates nothing, never synchronises the host and can be captured in a hipGraph.  real and fake
 * are dense float32 [B,K] in device memory; 4-byte alignment is enough (16-byte aligned bases with K % 4 == 0 take the vector
 * loads).
 *
 * Directions.  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with the key
 * (seed & 0xffffffff, seed >> 32) and the counter (q & 0xffffffff, q >> 32, p, 0), q = k / 4: its four words r0..r3 give the
 * elements k = 4q .. 4q+3 of direction p (a last group is truncated at K).  u(r) = ((r >> 9) + 0.5) 2^-23, in (0,1) and exact in
 * fp32; (z0, z1) = sqrt(-2 ln u(r0)) (cos, sin)(2 pi u(r1)), (z2, z3) likewise from (r2, r3).  Direction p depends on neither P
 * nor K.  The P x K matrix is never stored: the kernels generate it on chip, forward and backward.
 *
 * Value.  theta^_p = theta_p / |theta_p|_2, a[i,p] = <real_i, theta^_p>, b[j,p] = <fake_j, theta^_p>,
 *     SW2 = 1 / (P B) sum_p sum_r (a_(r),p - b_(r),p)^2,
 * (r) the ascending order, ties broken by the lower sample index.  The square, not its root (no gradient at 0).
 * Gradient for an upstream g: db[j,p] = -(2 g / (P B)) (a_(rank_b(j)),p - b[j,p]), da the mirror image;
 * dfake[j,k] = sum_p db[j,p] theta^_p[k], dreal likewise.
 *
 * Arithmetic.  Products and sums over k are fp32 inside a chunk of K (kccot_swd_plan), chunks are added in fp64 in a fixed order
 * and the sum, times 1 / |theta_p| in fp64, is rounded once; sum theta^2 is accumulated in the same pass.  The squared
 * differences are summed in fp64.  No floating-point atomics: two identical calls give identical bits.  Rows of real and fake go
 * through one instruction sequence: fake bit-equal to real gives SW2 == 0 and all-zero gradients exactly.  Non-finite inputs
 * are not handled.
 *
 * Every argument check comes before any launch: KCCOT_EINVAL for a NULL tensor or result (the backward needs dreal or dfake, not
 * both), a dimension < 1, p_begin < 0, an output overlapping an input or another output, a workspace that is not 16-byte
 * aligned; KCCOT_EUNSUPPORTED for B > 1024, P > 65535 (p_begin + p_count > 65535) or K > 2^40; KCCOT_EWORKSPACE for a NULL
 * workspace or ws_bytes < kccot_swd_workspace_bytes(B, K, P).
 */
#ifndef KCCOT_SWD_H
#define KCCOT_SWD_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

#define KCCOT_SWD_MAX_B 1024
#define KCCOT_SWD_MAX_P 65535

/* Bytes of workspace for the forward and the backward (0 for an argument outside the limits): the per-chunk partial projections
 * and squared norms with one double per projection (forward), the coefficient matrix [2 B, P rounded up to 64] (backward). */
size_t kccot_swd_workspace_bytes(int B, int64_t K, int P);

/* proj_out [2,P,B]: the normalised projections a (plane 0) and b (plane 1), projection-major; order_out [2,P,B]: the sample
 * index at every rank; inv_norm_out [P]: 1 / |theta_p|; swd_out [1]: SW2. */
int kccot_swd_fwd_f32(const float* real, const float* fake, int B, int64_t K, int P, uint64_t seed, float* proj_out,
                      int32_t* order_out, float* inv_norm_out, float* swd_out, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* dreal, dfake [B,K] (either may be NULL) from the forward's proj, order, inv_norm and the upstream gswd (one device float);
 * B, K, P and seed as in the forward call.  The videos are not read. */
int kccot_swd_bwd_f32(const float* gswd, const float* proj, const int32_t* order, const float* inv_norm, int B, int64_t K,
                      int P, uint64_t seed, float* dreal, float* dfake, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* out [p_count,K]: the raw (un-normalised) directions p_begin .. p_begin + p_count - 1. */
int kccot_swd_directions_f32(uint64_t seed, int64_t K, int p_begin, int p_count, float* out, kccot_stream_t stream);

/* The tiling of the three kernels at this shape: a pure host function (no device call, no GPU needed) that runs the planner of
 * the launches.  The argument rules of the entry points above that concern B, K and P, with the same codes (KCCOT_EINVAL also
 * for out == NULL).  out receives KCCOT_SWD_PLAN_INTS ints:
 *   [0] [1]  kc, chunks: the length of a K-chunk (fp32 inside, fp64 across) and their number
 *   [2] [3]  pt, rt: the projections and the rows of [real; fake] that one workgroup of swd_project holds
 *   [4] [5]  npt, nrt: projection tiles and row tiles (a row tile beyond the first regenerates its directions)
 *   [6]      np: the padded length of the bitonic sort (a power of two >= B)
 *   [7]      kt: the columns of one workgroup of swd_backproject */
#define KCCOT_SWD_PLAN_INTS 8
int kccot_swd_plan(int B, int64_t K, int P, int* out);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_SWD_H */
