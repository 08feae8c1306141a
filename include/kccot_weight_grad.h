/* kccot_weight_grad.h -- C ABI of the WEIGHT GRADIENTS of the weighted Sinkhorn solver (kccot_weighted.h) and of the
 * kernel-conditional loss (kccot_conditional.h) of libkccot.so: the entry points of those two headers "do not differentiate
 * the weights"; these do.  An EXTENSION, outside the versioned surface of kccot.h (KCCOT_VERSION).  Strict C99.  Error codes,
 * kccot_last_error(), kccot_stream_t and the cost flags are those of kccot.h; every call is asynchronous on `stream`,
 * allocates nothing, never synchronises the host and can be captured in a hipGraph.  All tensors are dense float32 in device
 * memory.
 *
 * In the loop of kccot_weighted.h, u_t = eps log a + (terms that do not depend on a directly) and v_t = eps log b + (...).
 * With gu_t the adjoint of u_t and gv_t the adjoint of v_t that the reverse sweep holds anyway (gv_nits: the final-cost
 * term; the adjoint of v_0 = 0, a constant, is not part of the sum):
 *     dW/da_i = (eps / a_i) sum_{t=1..nits} gu_t[i],          dW/db_j = (eps / b_j) sum_{t=1..nits} gv_t[j]
 * The sweep accumulates the two sums in double, one private entry per line, removes the conserved zero-sum mode of the
 * adjoints (its exact amplitude is zero; in fp32 a rounding residue that would be counted nits times) and scales once at
 * the end: no extra plan, no extra exponential, no extra pass over C.  The other outputs of a _dw call (dC, dC3, dfake,
 * feature gradients) hold the bits of the call without _dw.  When one vector feeds both marginals its gradient is da + db.
 * A problem the forward poisoned (nits < 0: a weight <= 0 or not finite) gets NaN da / db, like its dC.
 * On a rejected call (any code below, raised before any launch) every output is left untouched.
 */
#ifndef KCCOT_WEIGHT_GRAD_H
#define KCCOT_WEIGHT_GRAD_H

#include "kccot.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kccot_sinkhorn_weighted_bwd_f32 that also writes da_out, db_out [nprob,n]: row p = gcost[p] dW_p/da, gcost[p] dW_p/db.
 * Both are required.  Workspace and error codes as there; KCCOT_EINVAL also for a NULL da_out / db_out. */
int kccot_sinkhorn_weighted_bwd_dw_f32(const float* C, const float* a, const float* b, const float* u_hist,
                                       const float* v_hist, const int32_t* nits, int nprob, int n, float eps, int L,
                                       const float* gcost, float* dC_out, float* da_out, float* db_out, void* ws,
                                       size_t ws_bytes, kccot_stream_t stream);

/* kccot_weighted_sinkhorn_loss_bwd_f32 that also writes dw_real, dw_fake [B] (both required).  With da_k, db_k the weight
 * gradients of problem k of (xy, xx, yy), each already scaled by gloss {2,-1,-1}[k]:
 *     dw_real = da_xy + (da_xx + db_xx),      dw_fake = db_xy + (da_yy + db_yy)            (double, in that order)
 * ws: kccot_weighted_sinkhorn_loss_dw_workspace_bytes(B, K) bytes (the layout of the call without _dw, then da, db [3,B]).
 * KCCOT_EINVAL: as kccot_weighted_sinkhorn_loss_bwd_f32, and a NULL dw_real / dw_fake; KCCOT_EWORKSPACE: workspace too
 * small; KCCOT_EUNSUPPORTED: B > 1024. */
size_t kccot_weighted_sinkhorn_loss_dw_workspace_bytes(int B, int64_t K);
int kccot_weighted_sinkhorn_loss_bwd_dw_f32(const float* gloss, const float* real, const float* fake, int B, int64_t K,
                                            float sc, const float* h_fake, const float* h_real, const float* m_real,
                                            const float* m_fake, int T, int J, float eps, int L, const float* w_real,
                                            const float* w_fake, const float* C3, const float* u_hist, const float* v_hist,
                                            const int32_t* nits, float* dfake, float* dh_fake, float* dh_real,
                                            float* dm_real, float* dm_fake, float* dw_real, float* dw_fake, void* ws,
                                            size_t ws_bytes, kccot_stream_t stream);

/* kccot_sinkhorn_conditional_bwd_f32 that also writes the gradient w.r.t. the weight rows and the query weights.
 * cost [Q,3]: the forward's cost_out.  dw_out [Q,n] (required):
 *     dw_out[q] = sum_k (da_{3q+k} + db_{3q+k})         (double, k = 0, 1, 2; problem 3q+k carries gloss omega_q {2,-1,-1}[k])
 * domega_out [Q] (may be NULL): domega_out[q] = gloss (2 c_q0 - c_q1 - c_q2), in double -- also when omega is NULL (1/Q).
 * ws: kccot_sinkhorn_conditional_dw_workspace_bytes(Q, n) bytes: the layout of kccot_sinkhorn_conditional_bwd_f32, then the
 * per-problem da, db [3 Q,n].  A poisoned query has a NaN row of dw_out and a NaN domega_out; the other rows are those of a
 * clean run.  KCCOT_EINVAL, KCCOT_EWORKSPACE, KCCOT_EUNSUPPORTED as there, and KCCOT_EINVAL for a NULL cost / dw_out. */
size_t kccot_sinkhorn_conditional_dw_workspace_bytes(int Q, int n);
int kccot_sinkhorn_conditional_bwd_dw_f32(const float* gloss, const float* C3, const float* w, const float* omega,
                                          const float* u_hist, const float* v_hist, const int32_t* nits, int Q, int n,
                                          float eps, int L, float* dC3_out, const float* cost, float* dw_out,
                                          float* domega_out, void* ws, size_t ws_bytes, kccot_stream_t stream);

/* kccot_conditional_sinkhorn_loss_bwd_f32 with (cost, dw_out, domega_out) as above (n = B).
 * ws: kccot_conditional_sinkhorn_loss_dw_workspace_bytes(B, K, Q) bytes. */
size_t kccot_conditional_sinkhorn_loss_dw_workspace_bytes(int B, int64_t K, int Q);
int kccot_conditional_sinkhorn_loss_bwd_dw_f32(const float* gloss, const float* real, const float* fake, int B, int64_t K,
                                               float sc, const float* h_fake, const float* h_real, const float* m_real,
                                               const float* m_fake, int T, int J, float eps, int L, const float* w,
                                               const float* omega, int Q, const float* C3, const float* u_hist,
                                               const float* v_hist, const int32_t* nits, float* dfake, float* dh_fake,
                                               float* dh_real, float* dm_real, float* dm_fake, const float* cost,
                                               float* dw_out, float* domega_out, void* ws, size_t ws_bytes,
                                               kccot_stream_t stream);

/* Adjoint of kccot_conditional_weights_f32, from the STORED weights w [Q,n] and their upstream gradient dw [Q,n], one wave
 * per row.  The floor has zero slope, so floored entries (softmax mass < 2^-100) contribute nothing:
 *     live_qi = w_qi > 2^-100            m_q = sum_{live} w_qi dw_qi                        (double)
 *     dl_qi   = live ? w_qi (dw_qi - m_q) : 0
 *     dD_out[q,i] = -dl_qi / (2 bandwidth^2)           dbw_out[q] = sum_i dl_qi D_qi / bandwidth^3   (double, one float per row)
 * dD_out [Q,n] and dbw_out [Q] are both required; the caller adds the Q row terms of dbw_out.  A NaN weight counts as live
 * and gives a NaN row.  KCCOT_EINVAL: NULL pointer, Q < 1, n < 1, bandwidth not > 0; KCCOT_EUNSUPPORTED: n > 1024. */
int kccot_conditional_weights_bwd_f32(const float* D, const float* w, const float* dw, int Q, int n, float bandwidth,
                                      float* dD_out, float* dbw_out, kccot_stream_t stream);

/* The estimator and its adjoint with the bandwidth read from DEVICE memory (one float), for a bandwidth that is itself being
 * learned: no host read of it, so a step that uses it can be captured.  The same arithmetic as the calls that take the
 * bandwidth by value (the scale is formed in double from the same float: the same bits).  A bandwidth that is not > 0 cannot
 * be rejected on the host: it gives NaN weights (which the solver reports) and NaN gradients. */
int kccot_conditional_weights_dev_f32(const float* D, int Q, int n, const float* bandwidth, float* w_out,
                                      kccot_stream_t stream);
int kccot_conditional_weights_bwd_dev_f32(const float* D, const float* w, const float* dw, int Q, int n,
                                          const float* bandwidth, float* dD_out, float* dbw_out, kccot_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* KCCOT_WEIGHT_GRAD_H */
