/* kccot_conditional.h -- C ABI of the kernel-CONDITIONAL Sinkhorn loss of libkccot.so: Q weighted solves of the one-batch
 * loss on ONE shared set of cost matrices, and the kernel estimator that supplies their weights.
 * An EXTENSION, not reference behaviour: the reference evaluates the one-batch loss with mu = nu = 1/n only.  These entry
 * points are outside the versioned surface of kccot.h (KCCOT_VERSION).  Strict C99.  Error codes, kccot_last_error(),
 * kccot_stream_t and the cost flags are those of kccot.h; every call is asynchronous on `stream`, allocates nothing, never
 * synchronises the host and can be captured in a hipGraph.  All tensors are dense float32 in device memory.
 *
 * With C3 = [C_xy, C_xx, C_yy] (kccot_pairwise_cost3_f32), weight rows w [Q,n] (row q: the kernel estimate of the
 * conditional law given the context of query q; strictly positive, finite, normalised) and query weights omega [Q]
 * (NULL: 1/Q):
 *     loss_q = 2 W(C_xy; w_q, w_q) - W(C_xx; w_q, w_q) - W(C_yy; w_q, w_q)         W: the weighted loop of kccot_weighted.h
 *     loss   = sum_q omega_q loss_q                                                 (double accumulation, ascending q)
 * Real sample i and fake sample i share context i, so both marginals of all three problems are w_q.  The weights are
 * not differentiated here (kccot_weight_grad.h: dw, domega and the estimator's adjoint): dC3[k] = gloss sum_q omega_q {2,-1,-1}[k] dW_{q,k}/dC through the executed iterations (double
 * accumulation, ascending q: no result depends on the order in which workgroups finish).
 *
 * Problem p = 3 q + k reads cost matrix k of the shared C3 and weight row q; everything per problem (histories, costs,
 * counts) is indexed by p.  Dispatch: n <= 128 the register-resident weighted kernels, 128 < n <= 1024 the streaming
 * single-workgroup weighted solver (one transposed copy of C3 for all Q queries).  The multi-CU solver and the one-launch
 * fused loss are never selected.  A weight that is <= 0 or not finite poisons the three problems of ITS QUERY only: NaN
 * costs and nits = -1 for q, hence a NaN loss and NaN gradients; every other problem's outputs are bit for bit those of a
 * clean run.
 */
#ifndef KCCOT_CONDITIONAL_H
#define KCCOT_CONDITIONAL_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Kernel estimator of the conditional law from squared context distances D [Q,n] (D[q,i] = |c_q - c_i|^2):
 *     l_qi = -D_qi / (2 bandwidth^2),   w_qi = max(exp(l_qi - max_i l_q.) / sum_i exp(l_qi - max_i l_q.), 2^-100)
 * evaluated as exp2 of (min_i D_q. - D_qi) log2(e) / (2 bandwidth^2), one wave per row.  The floor 2^-100 (a normal fp32
 * number with an exact log2) keeps a peaked kernel from handing the solver a zero weight; the rows are NOT renormalised
 * after it.  Row sums of the stored weights: |sum_i w_qi - 1| <= 2^-22 for n <= 1024 (the denominator is summed in double
 * and rounded to fp32 once, each quotient is rounded once: 2^-24 each, with room for their product and the double sum's
 * own error; the floor adds at most n * 2^-100 <= 2^-90).  A NaN distance gives a row of NaN weights, which the solver
 * then reports.
 * KCCOT_EINVAL: NULL pointer, Q < 1, n < 1, bandwidth not > 0; KCCOT_EUNSUPPORTED: n > 1024. */
int kccot_conditional_weights_f32(const float* D, int Q, int n, float bandwidth, float* w_out, kccot_stream_t stream);

/* The 3 Q solves on the shared C3 [3,n,n] and their combination.  u_hist / v_hist [Q,3,max(L,1),n] are what the backward
 * needs; both may be NULL when no gradient is wanted (the costs are the same bits).  cost_out [Q,3]; nits_out [2][Q][3]:
 * reference-equivalent counts, then iterations executed; loss_out [1].  Count-based stop rule (KCCOT_STOP_COUNT).
 * Backward: gloss [1] on the device; dC3_out [3,n,n].  ws: kccot_sinkhorn_conditional_workspace_bytes(Q, n) bytes for
 * either direction (the backward keeps the 3 Q per-problem gradients and upstream factors there).
 * KCCOT_EINVAL, before any launch: a NULL required pointer, Q < 1, n < 1, eps <= 0, L < 0, u_hist / v_hist not given
 * together; KCCOT_EWORKSPACE: workspace too small; KCCOT_EUNSUPPORTED: n > 1024. */
size_t kccot_sinkhorn_conditional_workspace_bytes(int Q, int n);
int kccot_sinkhorn_conditional_fwd_f32(const float* C3, const float* w, const float* omega, int Q, int n, float eps, int L,
                                       int Lmin, float thresh, float* u_hist, float* v_hist, float* cost_out,
                                       int32_t* nits_out, float* loss_out, void* ws, size_t ws_bytes, kccot_stream_t stream);
int kccot_sinkhorn_conditional_bwd_f32(const float* gloss, const float* C3, const float* w, const float* omega,
                                       const float* u_hist, const float* v_hist, const int32_t* nits, int Q, int n,
                                       float eps, int L, float* dC3_out, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* The loss from videos and features: the arguments of kccot_weighted_sinkhorn_loss_fwd_f32 / _bwd_f32 with (w [Q,B],
 * omega [Q] or NULL, Q) in place of (w_real, w_fake), the outputs of the pair above, and no ticket.  These two only
 * sequence stages: forward = kccot_pairwise_cost3_f32 -> conditional forward (C3 [3,B,B] is an output the backward
 * reads); backward = conditional backward -> cost backward.  dfake, dh_fake, dh_real, dm_real, dm_fake: each may be NULL.
 * ws: kccot_conditional_sinkhorn_loss_workspace_bytes(B, K, Q) bytes.
 * KCCOT_EINVAL: as above, and B, K, T or J < 1; KCCOT_EWORKSPACE: workspace too small; KCCOT_EUNSUPPORTED: B > 1024. */
size_t kccot_conditional_sinkhorn_loss_workspace_bytes(int B, int64_t K, int Q);
int kccot_conditional_sinkhorn_loss_fwd_f32(const float* real, const float* fake, int B, int64_t K, float sc,
                                            const float* h_fake, const float* h_real, const float* m_real,
                                            const float* m_fake, int T, int J, float eps, int L, int Lmin, float thresh,
                                            unsigned flags, const float* w, const float* omega, int Q, float* C3,
                                            float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out,
                                            float* loss_out, void* ws, size_t ws_bytes, kccot_stream_t stream);
int kccot_conditional_sinkhorn_loss_bwd_f32(const float* gloss, const float* real, const float* fake, int B, int64_t K,
                                            float sc, const float* h_fake, const float* h_real, const float* m_real,
                                            const float* m_fake, int T, int J, float eps, int L, const float* w,
                                            const float* omega, int Q, const float* C3, const float* u_hist,
                                            const float* v_hist, const int32_t* nits, float* dfake, float* dh_fake,
                                            float* dh_real, float* dm_real, float* dm_fake, void* ws, size_t ws_bytes,
                                            kccot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_CONDITIONAL_H */
