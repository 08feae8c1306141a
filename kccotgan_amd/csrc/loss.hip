// compute_sinkhorn_loss (gan_utils.py:204-227) as ONE host call each way: the launch sequence
// cost assembly -> three Sinkhorn solves + combination (forward) and reverse sweep -> cost backward
// (backward) is issued from C, so a caller pays one FFI crossing and one workspace per direction
// instead of one per stage.  No new kernels (but the B-thread combination of the weight gradients at the end of the file):
// these entry points only sequence the stage functions.
// The bi-causal loss (bicausal.hip) runs the same sequence with one launch more in the forward (its second causal terms)
// and its own feature-gradient jobs in the cost backward.
#include "common.h"

namespace kccot {
static size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// cost assembly [-> bi-causal terms] -> the three solves + combination: ONE launch with the reverse sweep at dLoss = 1 when
// dC3_unit is given (C3 is then scratch for the caller), the dual history (u_hist / v_hist, both may be null) otherwise
static int loss3_fwd(bool bicausal, const float* real, const float* fake, int B, int64_t K, float sc, const float* h_fake,
                     const float* h_real, const float* m_real, const float* m_fake, int T, int J, float eps, int L, int Lmin,
                     float thresh, unsigned flags, float* C3, float* u_hist, float* v_hist, float* dC3_unit,
                     float* cost3_out, int32_t* nits_out, float* loss_out, int32_t* ticket, void* ws, size_t ws_bytes,
                     kccot_stream_t stream, const float* w_real = nullptr, const float* w_fake = nullptr) {
    if (flags & KCCOT_COST_BICAUSAL_TERM_ONLY)      // a step of the sharded caller's assembly, not a cost-ladder option
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fwd: KCCOT_COST_BICAUSAL_TERM_ONLY does not apply to a loss call");
    if (flags & KCCOT_COST_RBF_SUM)                 // the sharded kernel-MMD's step on a finished distance block
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fwd: KCCOT_COST_RBF_SUM does not apply to a loss call");
    int rc = kccot_pairwise_cost3_f32(real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, flags, C3, ws, ws_bytes,
                                      stream);
    if (rc) return rc;
    if (bicausal && (rc = launch_bicausal_cost_add(C3, B, h_fake, h_real, m_real, m_fake, T, J, sc, (hipStream_t)stream)))
        return rc;
    if (w_real)     // weighted marginals (kccot_weighted.h): the history path only, the fused launch is not weighted
        return sinkhorn_divergence_weighted_fwd(C3, w_real, w_fake, B, eps, L, Lmin, thresh, u_hist, v_hist, cost3_out,
                                                nits_out, loss_out, ticket, ws, ws_bytes, (hipStream_t)stream);
    if (dC3_unit)
        return kccot_sinkhorn_divergence_fused_f32(C3, B, eps, L, Lmin, thresh, cost3_out, nits_out, loss_out, ticket,
                                                   dC3_unit, stream);
    return kccot_sinkhorn_divergence_fwd_f32(C3, B, eps, L, Lmin, thresh, u_hist, v_hist, cost3_out, nits_out, loss_out,
                                             ticket, ws, ws_bytes, stream);
}

// after the fused forward: coefficient build (dC3_unit x gloss) -> video gradient; after the history forward: reverse sweep
// into the workspace, laid out dC3 [3,B,B] | 3 floats | stage, then the cost backward in the stage
static int loss3_bwd(bool bicausal, const float* gloss, const float* real, const float* fake, int B, int64_t K, float sc,
                     const float* h_fake, const float* h_real, const float* m_real, const float* m_fake, int T, int J,
                     float eps, int L, const float* C3, const float* u_hist, const float* v_hist, const int32_t* nits,
                     const float* dC3_unit, float* dfake, float* dh_fake, float* dh_real, float* dm_real, float* dm_fake,
                     void* ws, size_t ws_bytes, kccot_stream_t stream, const float* w_real = nullptr,
                     const float* w_fake = nullptr, float* da3 = nullptr, float* db3 = nullptr) {
    const hipStream_t st = (hipStream_t)stream;
    if (dC3_unit)
        return cost3_bwd_loss(dC3_unit, gloss, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, dfake, dh_fake,
                              dh_real, dm_real, dm_fake, ws, ws_bytes, st, bicausal);
    char* base = static_cast<char*>(ws);
    float* dC3 = reinterpret_cast<float*>(base);
    const size_t off_gc = up256((size_t)3 * B * B * sizeof(float));
    float* gc = reinterpret_cast<float*>(base + off_gc);
    void* stage = base + off_gc + 256;
    const size_t stage_bytes = ws_bytes - off_gc - 256;
    int rc;
    if (w_real) {
        rc = sinkhorn_divergence_weighted_bwd(C3, w_real, w_fake, u_hist, v_hist, nits, B, eps, L, gloss, gc, dC3, stage,
                                              stage_bytes, st, da3, db3);
    } else if (kccot_sinkhorn_workspace_bytes(3, B) > 0) {
        // streaming solver (n > 128): weights {2,-1,-1} * gloss first, then the generic reverse sweep
        rc = kccot_mixed_divergence_bwd_f32(gloss, gc, stream);
        if (rc) return rc;
        rc = kccot_sinkhorn_bwd_f32(C3, u_hist, v_hist, nits, 3, B, eps, L, gc, dC3, stage, stage_bytes, stream);
    } else {
        rc = kccot_sinkhorn_divergence_bwd_f32(C3, u_hist, v_hist, nits, B, eps, L, gloss, dC3, stage, stage_bytes, stream);
    }
    if (rc) return rc;
    return cost3_bwd_loss(dC3, nullptr, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, dfake, dh_fake, dh_real,
                          dm_real, dm_fake, stage, stage_bytes, st, bicausal);
}

// dw_real = da_xy + (da_xx + db_xx), dw_fake = db_xy + (da_yy + db_yy) from the per-problem weight gradients da3, db3 [3,B]
// of the weighted divergence (each already scaled by gloss {2,-1,-1}[k]); double, in that order
__global__ __launch_bounds__(256) void weighted_dw_combine(const float* __restrict__ da3, const float* __restrict__ db3, int B,
                                                           float* __restrict__ dw_real, float* __restrict__ dw_fake) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    dw_real[i] = (float)((double)da3[i] + ((double)da3[B + i] + (double)db3[B + i]));
    dw_fake[i] = (float)((double)db3[i] + ((double)da3[2 * B + i] + (double)db3[2 * B + i]));
}
}  // namespace kccot
using namespace kccot;

extern "C" size_t kccot_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    if (B <= 0 || K <= 0) return 0;
    // forward: cost stage | Sinkhorn stage;  backward: dC3 [3,B,B] + 3 floats, then Sinkhorn | cost-backward stage
    const size_t stage = max3(kccot_pairwise_cost3_workspace_bytes(B, K), kccot_sinkhorn_workspace_bytes(3, B),
                              kccot_pairwise_cost3_bwd_workspace_bytes(B, K));
    return up256((size_t)3 * B * B * sizeof(float)) + 256 + up256(stage);
}

extern "C" int kccot_sinkhorn_loss_fwd_f32(const float* real, const float* fake, int B, int64_t K, float sc,
                                           const float* h_fake, const float* h_real, const float* m_real,
                                           const float* m_fake, int T, int J, float eps, int L, int Lmin,
                                           float thresh, unsigned flags, float* C3, float* u_hist, float* v_hist,
                                           float* cost3_out, int32_t* nits_out, float* loss_out, int32_t* ticket,
                                           void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!C3 || !cost3_out || !nits_out || !loss_out || !ticket)
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fwd: null output pointer");
    if (ws_bytes < kccot_sinkhorn_loss_workspace_bytes(B, K) || (!ws && ws_bytes))
        return fail(KCCOT_EWORKSPACE, "sinkhorn_loss_fwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_fwd(false, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, Lmin, thresh, flags, C3,
                     u_hist, v_hist, nullptr, cost3_out, nits_out, loss_out, ticket, ws, ws_bytes, stream);
}

extern "C" int kccot_sinkhorn_loss_bwd_f32(const float* gloss, const float* real, const float* fake, int B, int64_t K,
                                           float sc, const float* h_fake, const float* h_real, const float* m_real,
                                           const float* m_fake, int T, int J, float eps, int L, const float* C3,
                                           const float* u_hist, const float* v_hist, const int32_t* nits,
                                           float* dfake, float* dh_fake, float* dh_real, float* dm_real, float* dm_fake,
                                           void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!gloss || !C3 || !u_hist || !v_hist || !nits) return fail(KCCOT_EINVAL, "sinkhorn_loss_bwd: null pointer");
    if (!ws || ws_bytes < kccot_sinkhorn_loss_workspace_bytes(B, K))
        return fail(KCCOT_EWORKSPACE, "sinkhorn_loss_bwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_bwd(false, gloss, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, C3, u_hist, v_hist,
                     nits, nullptr, dfake, dh_fake, dh_real, dm_real, dm_fake, ws, ws_bytes, stream);
}

// ---- the same with the fused solve + sweep (kccot_sinkhorn_divergence_fused_f32) ----------------------------------
// forward = cost assembly -> ONE launch (three solves, combination, reverse sweep at dLoss = 1): C3 is scratch for the
// caller, dC3_unit [3,B,B] is what the backward needs; backward = coefficient build (x gloss) -> video gradient.
extern "C" int kccot_sinkhorn_loss_fused_fwd_f32(const float* real, const float* fake, int B, int64_t K, float sc,
                                                 const float* h_fake, const float* h_real, const float* m_real,
                                                 const float* m_fake, int T, int J, float eps, int L, int Lmin,
                                                 float thresh, unsigned flags, float* C3, float* dC3_unit,
                                                 float* cost3_out, int32_t* nits_out, float* loss_out, int32_t* ticket,
                                                 void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!C3 || !dC3_unit || !cost3_out || !nits_out || !loss_out || !ticket)
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fused_fwd: null output pointer");
    if (ws_bytes < kccot_sinkhorn_loss_workspace_bytes(B, K) || (!ws && ws_bytes))
        return fail(KCCOT_EWORKSPACE, "sinkhorn_loss_fused_fwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_fwd(false, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, Lmin, thresh, flags, C3,
                     nullptr, nullptr, dC3_unit, cost3_out, nits_out, loss_out, ticket, ws, ws_bytes, stream);
}

extern "C" int kccot_sinkhorn_loss_fused_bwd_f32(const float* gloss, const float* dC3_unit, const float* real,
                                                 const float* fake, int B, int64_t K, float sc, const float* h_fake,
                                                 const float* h_real, const float* m_real, const float* m_fake, int T, int J,
                                                 float* dfake, float* dh_fake, float* dh_real, float* dm_real, float* dm_fake,
                                                 void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!gloss || !dC3_unit) return fail(KCCOT_EINVAL, "sinkhorn_loss_fused_bwd: null pointer");
    return loss3_bwd(false, gloss, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, 0.f, 0, nullptr, nullptr,
                     nullptr, nullptr, dC3_unit, dfake, dh_fake, dh_real, dm_real, dm_fake, ws, ws_bytes, stream);
}

// ---- the bi-causal loss (bicausal.hip) -------------------------------------------------------------------------------
extern "C" size_t kccot_bicausal_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    // the one-batch loss's layout: dC3 [3,B,B] + 3 floats of the history backward, then one stage at a time
    return kccot_sinkhorn_loss_workspace_bytes(B, K);
}

extern "C" int kccot_bicausal_sinkhorn_loss_fwd_f32(const float* real, const float* fake, int B, int64_t K, float sc,
                                                    const float* h_fake, const float* h_real, const float* m_real,
                                                    const float* m_fake, int T, int J, float eps, int L, int Lmin,
                                                    float thresh, unsigned flags, float* C3, float* u_hist, float* v_hist,
                                                    float* dC3_unit, float* cost3_out, int32_t* nits_out, float* loss_out,
                                                    int32_t* ticket, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!real || !fake || !h_fake || !h_real || !m_real || !m_fake)
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_fwd: null input pointer");
    if (!C3 || !cost3_out || !nits_out || !loss_out || !ticket)
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_fwd: null output pointer");
    if (B <= 0 || K <= 0 || T < 1 || J < 1 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_fwd: bad arguments B=%d K=%lld T=%d J=%d L=%d eps=%g", B,
                    (long long)K, T, J, L, (double)eps);
    if ((u_hist == nullptr) != (v_hist == nullptr) || (dC3_unit && u_hist))
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_fwd: give u_hist and v_hist together, or dC3_unit, not both");
    if (flags & (KCCOT_COST_GRAM_SUMS_ONLY | KCCOT_COST_FROM_GRAM_SUMS))
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_fwd: the Gram-sum split flags do not apply");
    if (!ws || ws_bytes < kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K))
        return fail(KCCOT_EWORKSPACE, "bicausal_sinkhorn_loss_fwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_fwd(true, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, Lmin, thresh, flags, C3,
                     u_hist, v_hist, dC3_unit, cost3_out, nits_out, loss_out, ticket, ws, ws_bytes, stream);
}

extern "C" int kccot_bicausal_sinkhorn_loss_bwd_f32(const float* gloss, const float* real, const float* fake, int B,
                                                    int64_t K, float sc, const float* h_fake, const float* h_real,
                                                    const float* m_real, const float* m_fake, int T, int J, float eps,
                                                    int L, const float* C3, const float* u_hist, const float* v_hist,
                                                    const int32_t* nits, const float* dC3_unit, float* dfake,
                                                    float* dh_fake, float* dh_real, float* dm_real, float* dm_fake,
                                                    void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!gloss || !real || !fake || !h_fake || !h_real || !m_real || !m_fake)
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_bwd: null input pointer");
    if (!dC3_unit && (!C3 || !u_hist || !v_hist || !nits))
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_bwd: give dC3_unit (fused forward) or C3, u_hist, v_hist, nits");
    if (B <= 0 || K <= 0 || T < 1 || J < 1 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "bicausal_sinkhorn_loss_bwd: bad arguments B=%d K=%lld T=%d J=%d", B, (long long)K, T, J);
    if (!ws || ws_bytes < kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K))
        return fail(KCCOT_EWORKSPACE, "bicausal_sinkhorn_loss_bwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_bwd(true, gloss, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, C3, u_hist, v_hist,
                     nits, dC3_unit, dfake, dh_fake, dh_real, dm_real, dm_fake, ws, ws_bytes, stream);
}

// ---- the one-batch loss with weighted marginals (include/kccot_weighted.h) -------------------------------------------
// 2 W(C_xy; a, b) - W(C_xx; a, a) - W(C_yy; b, b) with a = w_real, b = w_fake: the launch sequence of
// kccot_sinkhorn_loss_fwd_f32 / _bwd_f32 on the dual-history path with the weighted solver kernels.  An EXTENSION: the
// reference's compute_sinkhorn hard-codes uniform marginals.
extern "C" size_t kccot_weighted_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    return kccot_sinkhorn_loss_workspace_bytes(B, K);
}

extern "C" int kccot_weighted_sinkhorn_loss_fwd_f32(const float* real, const float* fake, int B, int64_t K, float sc,
                                                    const float* h_fake, const float* h_real, const float* m_real,
                                                    const float* m_fake, int T, int J, float eps, int L, int Lmin,
                                                    float thresh, unsigned flags, const float* w_real, const float* w_fake,
                                                    float* C3, float* u_hist, float* v_hist, float* cost3_out,
                                                    int32_t* nits_out, float* loss_out, int32_t* ticket, void* ws,
                                                    size_t ws_bytes, kccot_stream_t stream) {
    if (!real || !fake || !h_fake || !h_real || !m_real || !m_fake || !w_real || !w_fake)
        return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_fwd: null input pointer");
    if (!C3 || !cost3_out || !nits_out || !loss_out || !ticket)
        return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_fwd: null output pointer");
    if (B <= 0 || K <= 0 || T < 1 || J < 1 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_fwd: bad arguments B=%d K=%lld T=%d J=%d L=%d eps=%g", B,
                    (long long)K, T, J, L, (double)eps);
    if ((u_hist == nullptr) != (v_hist == nullptr))
        return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_fwd: u_hist and v_hist must be given together");
    if (!ws || ws_bytes < kccot_weighted_sinkhorn_loss_workspace_bytes(B, K))
        return fail(KCCOT_EWORKSPACE, "weighted_sinkhorn_loss_fwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_weighted_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_fwd(false, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, Lmin, thresh, flags, C3,
                     u_hist, v_hist, nullptr, cost3_out, nits_out, loss_out, ticket, ws, ws_bytes, stream, w_real, w_fake);
}

extern "C" int kccot_weighted_sinkhorn_loss_bwd_f32(const float* gloss, const float* real, const float* fake, int B,
                                                    int64_t K, float sc, const float* h_fake, const float* h_real,
                                                    const float* m_real, const float* m_fake, int T, int J, float eps,
                                                    int L, const float* w_real, const float* w_fake, const float* C3,
                                                    const float* u_hist, const float* v_hist, const int32_t* nits,
                                                    float* dfake, float* dh_fake, float* dh_real, float* dm_real,
                                                    float* dm_fake, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!gloss || !real || !fake || !h_fake || !h_real || !m_real || !m_fake || !w_real || !w_fake)
        return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_bwd: null input pointer");
    if (!C3 || !u_hist || !v_hist || !nits) return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_bwd: null pointer");
    if (B <= 0 || K <= 0 || T < 1 || J < 1 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "weighted_sinkhorn_loss_bwd: bad arguments B=%d K=%lld T=%d J=%d", B, (long long)K, T, J);
    if (!ws || ws_bytes < kccot_weighted_sinkhorn_loss_workspace_bytes(B, K))
        return fail(KCCOT_EWORKSPACE, "weighted_sinkhorn_loss_bwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_weighted_sinkhorn_loss_workspace_bytes(B, K));
    return loss3_bwd(false, gloss, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, C3, u_hist, v_hist,
                     nits, nullptr, dfake, dh_fake, dh_real, dm_real, dm_fake, ws, ws_bytes, stream, w_real, w_fake);
}

// ---- the same backward with the gradient w.r.t. the two weight vectors (include/kccot_weight_grad.h) --------------------
// workspace: the layout of kccot_weighted_sinkhorn_loss_bwd_f32, then da3 | db3 [3,B] each
extern "C" size_t kccot_weighted_sinkhorn_loss_dw_workspace_bytes(int B, int64_t K) {
    const size_t base = kccot_weighted_sinkhorn_loss_workspace_bytes(B, K);
    return base ? base + up256((size_t)6 * B * sizeof(float)) : 0;
}

extern "C" int kccot_weighted_sinkhorn_loss_bwd_dw_f32(const float* gloss, const float* real, const float* fake, int B,
                                                       int64_t K, float sc, const float* h_fake, const float* h_real,
                                                       const float* m_real, const float* m_fake, int T, int J, float eps,
                                                       int L, const float* w_real, const float* w_fake, const float* C3,
                                                       const float* u_hist, const float* v_hist, const int32_t* nits,
                                                       float* dfake, float* dh_fake, float* dh_real, float* dm_real,
                                                       float* dm_fake, float* dw_real, float* dw_fake, void* ws,
                                                       size_t ws_bytes, kccot_stream_t stream) {
    const char* who = "weighted_sinkhorn_loss_bwd_dw";
    if (!gloss || !real || !fake || !h_fake || !h_real || !m_real || !m_fake || !w_real || !w_fake)
        return fail(KCCOT_EINVAL, "%s: null input pointer", who);
    if (!C3 || !u_hist || !v_hist || !nits) return fail(KCCOT_EINVAL, "%s: null pointer", who);
    if (!dw_real || !dw_fake) return fail(KCCOT_EINVAL, "%s: null dw_real / dw_fake", who);
    if (B <= 0 || K <= 0 || T < 1 || J < 1 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "%s: bad arguments B=%d K=%lld T=%d J=%d L=%d eps=%g", who, B, (long long)K, T, J, L,
                    (double)eps);
    if (B > 1024) return fail(KCCOT_EUNSUPPORTED, "%s: B=%d > 1024", who, B);
    const size_t need = kccot_weighted_sinkhorn_loss_dw_workspace_bytes(B, K);
    if (!ws || ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    const size_t base = kccot_weighted_sinkhorn_loss_workspace_bytes(B, K);
    float* da3 = reinterpret_cast<float*>(static_cast<char*>(ws) + base);
    float* db3 = da3 + (size_t)3 * B;
    int rc = loss3_bwd(false, gloss, real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L, C3, u_hist, v_hist,
                       nits, nullptr, dfake, dh_fake, dh_real, dm_real, dm_fake, ws, base, stream, w_real, w_fake, da3, db3);
    if (rc) return rc;
    hipLaunchKernelGGL(weighted_dw_combine, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)da3,
                       (const float*)db3, B, dw_real, dw_fake);
    return launch_status("weighted_dw_combine");
}
