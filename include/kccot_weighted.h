/* kccot_weighted.h -- C ABI of the Sinkhorn solver and the one-batch causal loss of libkccot.so with WEIGHTED marginals.
 * An EXTENSION: the reference's compute_sinkhorn hard-codes mu = nu = 1/n, and so does every entry point of
 * include/kccot.h.  These entry points are outside that header's versioned surface (KCCOT_VERSION).  Strict C99.  Error
 * codes, kccot_last_error(), kccot_stream_t, KCCOT_STOP_* and the cost flags are those of kccot.h; every call is
 * asynchronous on `stream`, allocates nothing, never synchronises the host and can be captured in a hipGraph.  All
 * tensors are dense float32 in device memory.
 *
 * Given an n x n cost C and weight vectors a, b (strictly positive, finite, normalised by the caller):
 *     u = v = 0; repeat up to L times (stop rule of kccot_sinkhorn_fwd_f32):
 *         u_i += eps (log a_i - LSE_j((-C_ij + u_i + v_j)/eps))
 *         v_j += eps (log b_j - LSE_i((-C_ij + u_i + v_j)/eps))
 *     W(C; a, b) = sum_ij exp((-C_ij + u_i + v_j)/eps) C_ij
 * With a = b = 1/n this is kccot_sinkhorn_fwd_f32 (to rounding: log(1/n) is then formed from the stored weights).
 * The weights are not differentiated by these entry points (kccot_weight_grad.h has the ones that do).  A weight that is <= 0 or not finite poisons ITS problem, not the launch:
 * cost = NaN, nits_out[p] = -1 (kccot_sinkhorn_status reports it), NaN gradients from the reverse sweep.
 * Dispatch: n <= 128 the register-resident kernels, 128 < n <= 1024 the streaming single-workgroup solver.  The
 * multi-CU solver (option sinkhorn_coop) and the one-launch fused loss (option sinkhorn_fused) are not weighted and are
 * never selected by these entry points.
 */
#ifndef KCCOT_WEIGHTED_H
#define KCCOT_WEIGHTED_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kccot_sinkhorn_fwd_f32 / kccot_sinkhorn_bwd_f32 with marginals a [nprob,n] (rows) and b [nprob,n] (columns); every
 * other argument, the outputs and the workspace (kccot_sinkhorn_workspace_bytes(nprob, n)) as there.
 * KCCOT_EINVAL: a NULL a or b and everything kccot_sinkhorn_fwd_f32 / _bwd_f32 reject, before any launch;
 * KCCOT_EWORKSPACE: workspace too small (n > 128); KCCOT_EUNSUPPORTED: n > 1024. */
int kccot_sinkhorn_weighted_fwd_f32(const float* C, const float* a, const float* b, int nprob, int n, float eps, int L,
                                    int Lmin, float thresh, int stop_mode, float* u_hist, float* v_hist, float* cost_out,
                                    int32_t* nits_out, float* pi_out, void* ws, size_t ws_bytes, kccot_stream_t stream);
int kccot_sinkhorn_weighted_bwd_f32(const float* C, const float* a, const float* b, const float* u_hist,
                                    const float* v_hist, const int32_t* nits, int nprob, int n, float eps, int L,
                                    const float* gcost, float* dC_out, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* loss = 2 W(C_xy; a, b) - W(C_xx; a, a) - W(C_yy; b, b), a = w_real [B], b = w_fake [B], with the three cost matrices
 * of kccot_sinkhorn_loss_fwd_f32: the arguments of kccot_sinkhorn_loss_fwd_f32 / _bwd_f32 plus the two weight vectors.
 * Forward: cost assembly -> weighted solves -> combination (the dual history u_hist / v_hist [3,max(L,1),B] is what the
 * backward needs; both may be NULL when no gradient is wanted).  Backward: weighted reverse sweeps -> cost backward.
 * `ticket`: one device int, zero on entry, left zero.  ws: kccot_weighted_sinkhorn_loss_workspace_bytes(B, K) bytes.
 * KCCOT_EINVAL: a NULL pointer (other than u_hist / v_hist of the forward, and gradient outputs that are not wanted),
 * B, K, T or J < 1, L < 0, eps <= 0; KCCOT_EWORKSPACE: workspace too small. */
size_t kccot_weighted_sinkhorn_loss_workspace_bytes(int B, int64_t K);
int kccot_weighted_sinkhorn_loss_fwd_f32(const float* real, const float* fake, int B, int64_t K, float sc,
                                         const float* h_fake, const float* h_real, const float* m_real,
                                         const float* m_fake, int T, int J, float eps, int L, int Lmin, float thresh,
                                         unsigned flags, const float* w_real, const float* w_fake, float* C3,
                                         float* u_hist, float* v_hist, float* cost3_out, int32_t* nits_out,
                                         float* loss_out, int32_t* ticket, void* ws, size_t ws_bytes,
                                         kccot_stream_t stream);
int kccot_weighted_sinkhorn_loss_bwd_f32(const float* gloss, const float* real, const float* fake, int B, int64_t K,
                                         float sc, const float* h_fake, const float* h_real, const float* m_real,
                                         const float* m_fake, int T, int J, float eps, int L, const float* w_real,
                                         const float* w_fake, const float* C3, const float* u_hist, const float* v_hist,
                                         const int32_t* nits, float* dfake, float* dh_fake, float* dh_real,
                                         float* dm_real, float* dm_fake, void* ws, size_t ws_bytes, kccot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_WEIGHTED_H */
