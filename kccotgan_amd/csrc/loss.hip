// compute_sinkhorn_loss (gan_utils.py:204-227) as ONE host call each way: the launch sequence cost assembly -> three Sinkhorn
// solves + combination (forward) and reverse sweep -> cost backward (backward) is issued from C, so a caller pays one FFI
// crossing and one workspace per direction instead of one per stage.  No new kernels (but the B-thread combination of the
// weight gradients below): these entry points only validate (loss_check) and sequence the stage functions (loss3_fwd / _bwd).
// The bi-causal loss (bicausal.hip) runs the same sequence with one launch more in the forward (its second causal terms) and
// its own feature-gradient jobs in the cost backward; the weighted loss (kccot_weighted.h) and the kernel-conditional loss
// (kccot_conditional.h; conditional.hip) run it with their own solver stage.
#include "common.h"

// the parameters every loss entry point shares, as the headers declare them: the videos [B,K] and the four features [B,T,J]
#define LOSS_INPUTS                                                                                                          \
    const float* real, const float* fake, int B, int64_t K, float sc, const float* h_fake, const float* h_real,              \
        const float* m_real, const float* m_fake, int T, int J

namespace kccot {
// LOSS_INPUTS and the solver's eps, L past the entry point
struct LossArgs {
    const float *real, *fake;
    int B;
    int64_t K;
    float sc;
    const float *h_fake, *h_real, *m_real, *m_fake;
    int T, J;
    float eps;
    int L;
};
struct LossGrads { float *dfake, *dh_fake, *dh_real, *dm_real, *dm_fake; };

// the marginals of the three problems (a null: uniform) and, in a weight-gradient backward (kccot_weight_grad.h), their gradient
//   weighted loss (Q = 0):      a = w_real, b = w_fake [B];  da | db: scratch [3,B] each for the per-problem gradients
//   conditional loss (Q >= 1):  a = w [Q,B], b = omega [Q] (null: 1/Q);  da = dw [Q,B], db = domega [Q] (may be null), from
//                               cost, the forward's costs [Q,3]
struct Weights {
    const float *a = nullptr, *b = nullptr;
    int Q = 0;
    float *da = nullptr, *db = nullptr;
    const float* cost = nullptr;
};

// workspace of a loss call: dC3 [3,B,B] of the history backward | gc: 256 B for gloss {2,-1,-1} (not in the conditional
// loss: its solver stage holds the 3 Q of them) | ONE stage at a time (cost assembly | solver | cost backward).  The forward
// uses the whole of it as its stage.
struct LossWs { size_t off_gc, off_stage; };
static LossWs loss_ws(int B, bool conditional) {
    const size_t off_gc = up256((size_t)3 * B * B * sizeof(float));
    return LossWs{off_gc, off_gc + (conditional ? 0 : 256)};
}
static size_t loss_ws_bytes(int B, int64_t K, bool conditional, size_t solver) {
    return loss_ws(B, conditional).off_stage +
           up256(max3(kccot_pairwise_cost3_workspace_bytes(B, K), solver, kccot_pairwise_cost3_bwd_workspace_bytes(B, K)));
}
// the solver stage of the conditional loss: zero outside the solver's limits (conditional.hip); dw: with its da | db
static size_t cond_loss_ws_bytes(int B, int64_t K, int Q, bool dw) {
    const size_t solver =
        dw ? kccot_sinkhorn_conditional_dw_workspace_bytes(Q, B) : kccot_sinkhorn_conditional_workspace_bytes(Q, B);
    return K < 1 || !solver ? 0 : loss_ws_bytes(B, K, true, solver);
}
// the weighted _dw backward keeps da3 | db3 [3,B] each behind the one-batch layout
static size_t weighted_dw_bytes(int B) { return up256((size_t)6 * B * sizeof(float)); }

// What loss_check validates for an entry point, in this order: KCCOT_EINVAL (pointers, shapes, history, flags),
// KCCOT_EUNSUPPORTED (the limits), KCCOT_EWORKSPACE
enum WsRule { WS_UNCHECKED, WS_NULL_IF_EMPTY, WS_REQUIRED };
struct LossCheck {
    bool inputs;                    // the videos, features and shapes are checked here (false: by the cost stage, which needs
                                    // no features)
    bool ptrs;                      // every other pointer the entry point requires is given
    bool hist = true;               // u_hist, v_hist [and dC3_unit] come in a combination the entry point takes
    unsigned refused = 0;           // the cost flags of the call that do not apply to it
    const int* queries = nullptr;   // given: the conditional solver's limits for *queries queries on B samples (conditional.hip)
    int max_B = 0;                  // > 0: a limit on B of the entry point's own
    WsRule ws;
    size_t need = 0;
};

static int loss_check(const char* who, const LossArgs& a, const LossCheck& c, const void* ws, size_t ws_bytes) {
    if (!c.ptrs || (c.inputs && (!a.real || !a.fake || !a.h_fake || !a.h_real || !a.m_real || !a.m_fake)))
        return fail(KCCOT_EINVAL, "%s: null pointer", who);
    if (c.inputs && (a.B < 1 || a.K < 1 || a.T < 1 || a.J < 1 || a.L < 0 || !(a.eps > 0.f)))
        return fail(KCCOT_EINVAL, "%s: bad arguments B=%d K=%lld T=%d J=%d L=%d eps=%g", who, a.B, (long long)a.K, a.T, a.J,
                    a.L, (double)a.eps);
    if (!c.hist)
        return fail(KCCOT_EINVAL, "%s: u_hist and v_hist must be given together (or, where it is a parameter, dC3_unit alone)",
                    who);
    if (c.refused) return fail(KCCOT_EINVAL, "%s: flags 0x%x do not apply to a loss call", who, c.refused);
    if (int rc = !c.queries ? 0 : cond_check(who, *c.queries, a.B, a.eps, a.L)) return rc;
    if (c.max_B && a.B > c.max_B) return fail(KCCOT_EUNSUPPORTED, "%s: B=%d > %d", who, a.B, c.max_B);
    if (c.ws != WS_UNCHECKED && (ws_bytes < c.need || (c.ws == WS_REQUIRED ? !ws : !ws && ws_bytes)))
        return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, c.need);
    return 0;
}

// cost assembly [-> bi-causal terms] -> the solves + combination: ONE launch with the reverse sweep at dLoss = 1 when
// dC3_unit is given (C3 is then scratch for the caller), the dual history (u_hist / v_hist, both may be null) otherwise;
// weighted marginals run the history path only (the fused launch is not weighted)
static int loss3_fwd(bool bicausal, const LossArgs& a, int Lmin, float thresh, unsigned flags, float* C3, float* u_hist,
                     float* v_hist, float* dC3_unit, float* cost_out, int32_t* nits_out, float* loss_out, int32_t* ticket,
                     void* ws, size_t ws_bytes, kccot_stream_t stream, const Weights& w = Weights()) {
    const hipStream_t st = (hipStream_t)stream;
    if (flags & KCCOT_COST_BICAUSAL_TERM_ONLY)      // a step of the sharded caller's assembly, not a cost-ladder option
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fwd: KCCOT_COST_BICAUSAL_TERM_ONLY does not apply to a loss call");
    if (flags & KCCOT_COST_RBF_SUM)                 // the sharded kernel-MMD's step on a finished distance block
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fwd: KCCOT_COST_RBF_SUM does not apply to a loss call");
    if (flags & KCCOT_COST_L1)                      // the one-call losses differentiate the squared cost only (kccot_l1.h)
        return fail(KCCOT_EINVAL, "sinkhorn_loss_fwd: KCCOT_COST_L1 does not apply to a loss call (its backward is the squared cost's)");
    int rc = kccot_pairwise_cost3_f32(a.real, a.fake, a.B, a.K, a.sc, a.h_fake, a.h_real, a.m_real, a.m_fake, a.T, a.J, flags,
                                      C3, ws, ws_bytes, stream);
    if (rc) return rc;
    if (bicausal && (rc = launch_bicausal_cost_add(C3, a.B, a.h_fake, a.h_real, a.m_real, a.m_fake, a.T, a.J, a.sc, st)))
        return rc;
    if (w.Q)
        return cond_fwd(C3, w.a, w.b, w.Q, a.B, a.eps, a.L, Lmin, thresh, u_hist, v_hist, cost_out, nits_out, loss_out, ws, st);
    if (w.a)
        return sinkhorn_divergence_weighted_fwd(C3, w.a, w.b, a.B, a.eps, a.L, Lmin, thresh, u_hist, v_hist, cost_out, nits_out,
                                                loss_out, ticket, ws, ws_bytes, st);
    if (dC3_unit)
        return kccot_sinkhorn_divergence_fused_f32(C3, a.B, a.eps, a.L, Lmin, thresh, cost_out, nits_out, loss_out, ticket,
                                                   dC3_unit, stream);
    return kccot_sinkhorn_divergence_fwd_f32(C3, a.B, a.eps, a.L, Lmin, thresh, u_hist, v_hist, cost_out, nits_out, loss_out,
                                             ticket, ws, ws_bytes, stream);
}

// after the fused forward: coefficient build (dC3_unit x gloss) -> video gradient in the whole workspace; after the history
// forward: reverse sweep into the workspace (LossWs), then the cost backward in its stage
static int loss3_bwd(bool bicausal, const float* gloss, const LossArgs& a, const float* C3, const float* u_hist,
                     const float* v_hist, const int32_t* nits, const float* dC3_unit, const LossGrads& g, void* ws,
                     size_t ws_bytes, kccot_stream_t stream, const Weights& w = Weights()) {
    const hipStream_t st = (hipStream_t)stream;
    const float *dC3 = dC3_unit, *gscale = gloss;
    void* stage = ws;
    size_t stage_bytes = ws_bytes;
    if (!dC3_unit) {
        const LossWs l = loss_ws(a.B, w.Q != 0);
        char* base = static_cast<char*>(ws);
        float* dC = reinterpret_cast<float*>(base);
        float* gc = reinterpret_cast<float*>(base + l.off_gc);
        stage = base + l.off_stage;
        stage_bytes = ws_bytes - l.off_stage;
        int rc;
        if (w.Q) {
            rc = cond_bwd(gloss, C3, w.a, w.b, u_hist, v_hist, nits, w.Q, a.B, a.eps, a.L, dC, stage, st, w.cost, w.da, w.db);
        } else if (w.a) {
            rc = sinkhorn_divergence_weighted_bwd(C3, w.a, w.b, u_hist, v_hist, nits, a.B, a.eps, a.L, gloss, gc, dC, stage,
                                                  stage_bytes, st, w.da, w.db);
        } else if (kccot_sinkhorn_workspace_bytes(3, a.B) > 0) {
            // streaming solver (n > 128): weights {2,-1,-1} * gloss first, then the generic reverse sweep
            rc = kccot_mixed_divergence_bwd_f32(gloss, gc, stream);
            if (rc) return rc;
            rc = kccot_sinkhorn_bwd_f32(C3, u_hist, v_hist, nits, 3, a.B, a.eps, a.L, gc, dC, stage, stage_bytes, stream);
        } else {
            rc = kccot_sinkhorn_divergence_bwd_f32(C3, u_hist, v_hist, nits, a.B, a.eps, a.L, gloss, dC, stage, stage_bytes,
                                                   stream);
        }
        if (rc) return rc;
        dC3 = dC;
        gscale = nullptr;
    }
    return cost3_bwd_loss(dC3, gscale, a.real, a.fake, a.B, a.K, a.sc, a.h_fake, a.h_real, a.m_real, a.m_fake, a.T, a.J,
                          g.dfake, g.dh_fake, g.dh_real, g.dm_real, g.dm_fake, stage, stage_bytes, st, bicausal);
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

// the weighted backward, with the gradient w.r.t. the two weight vectors when dw_real / dw_fake are given
static int weighted_loss_bwd(const char* who, const float* gloss, const LossArgs& a, const float* w_real, const float* w_fake,
                             const float* C3, const float* u_hist, const float* v_hist, const int32_t* nits,
                             const LossGrads& g, float* dw_real, float* dw_fake, void* ws, size_t ws_bytes,
                             kccot_stream_t stream) {
    const bool dw = dw_real != nullptr;
    const size_t base = kccot_weighted_sinkhorn_loss_workspace_bytes(a.B, a.K);
    const LossCheck c{.inputs = true, .ptrs = gloss && w_real && w_fake && C3 && u_hist && v_hist && nits,
                      .max_B = dw ? 1024 : 0, .ws = WS_REQUIRED, .need = dw ? base + weighted_dw_bytes(a.B) : base};
    int rc = loss_check(who, a, c, ws, ws_bytes);
    if (rc) return rc;
    float* da3 = dw ? reinterpret_cast<float*>(static_cast<char*>(ws) + base) : nullptr;      // da3 | db3 behind the layout
    float* db3 = dw ? da3 + (size_t)3 * a.B : nullptr;
    rc = loss3_bwd(false, gloss, a, C3, u_hist, v_hist, nits, nullptr, g, ws, dw ? base : ws_bytes, stream,
                   Weights{w_real, w_fake, 0, da3, db3});
    if (rc || !dw) return rc;
    hipLaunchKernelGGL(weighted_dw_combine, dim3((a.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, (const float*)da3,
                       (const float*)db3, a.B, dw_real, dw_fake);
    return launch_status("weighted_dw_combine");
}

// the conditional backward, with the gradients w.r.t. the weight rows and the query weights when dw_out is given
static int conditional_loss_bwd(const char* who, const float* gloss, const LossArgs& a, const float* w, const float* omega,
                                int Q, const float* C3, const float* u_hist, const float* v_hist, const int32_t* nits,
                                const LossGrads& g, const float* cost, float* dw_out, float* domega_out, void* ws,
                                size_t ws_bytes, kccot_stream_t stream) {
    const LossCheck c{.inputs = true, .ptrs = gloss && w && C3 && u_hist && v_hist && nits, .queries = &Q, .ws = WS_REQUIRED,
                      .need = cond_loss_ws_bytes(a.B, a.K, Q, dw_out != nullptr)};
    if (int rc = loss_check(who, a, c, ws, ws_bytes)) return rc;
    return loss3_bwd(false, gloss, a, C3, u_hist, v_hist, nits, nullptr, g, ws, ws_bytes, stream,
                     Weights{w, omega, Q, dw_out, domega_out, cost});
}
}  // namespace kccot
using namespace kccot;

extern "C" size_t kccot_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    if (B <= 0 || K <= 0) return 0;
    return loss_ws_bytes(B, K, false, kccot_sinkhorn_workspace_bytes(3, B));
}

extern "C" int kccot_sinkhorn_loss_fwd_f32(LOSS_INPUTS, float eps, int L, int Lmin, float thresh, unsigned flags, float* C3,
                                           float* u_hist, float* v_hist, float* cost3_out, int32_t* nits_out, float* loss_out,
                                           int32_t* ticket, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const LossCheck c{.inputs = false, .ptrs = C3 && cost3_out && nits_out && loss_out && ticket, .ws = WS_NULL_IF_EMPTY,
                      .need = kccot_sinkhorn_loss_workspace_bytes(B, K)};
    if (int rc = loss_check("sinkhorn_loss_fwd", a, c, ws, ws_bytes)) return rc;
    return loss3_fwd(false, a, Lmin, thresh, flags, C3, u_hist, v_hist, nullptr, cost3_out, nits_out, loss_out, ticket, ws,
                     ws_bytes, stream);
}

extern "C" int kccot_sinkhorn_loss_bwd_f32(const float* gloss, LOSS_INPUTS, float eps, int L, const float* C3,
                                           const float* u_hist, const float* v_hist, const int32_t* nits, float* dfake,
                                           float* dh_fake, float* dh_real, float* dm_real, float* dm_fake, void* ws,
                                           size_t ws_bytes, kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const LossCheck c{.inputs = false, .ptrs = gloss && C3 && u_hist && v_hist && nits, .ws = WS_REQUIRED,
                      .need = kccot_sinkhorn_loss_workspace_bytes(B, K)};
    if (int rc = loss_check("sinkhorn_loss_bwd", a, c, ws, ws_bytes)) return rc;
    return loss3_bwd(false, gloss, a, C3, u_hist, v_hist, nits, nullptr, {dfake, dh_fake, dh_real, dm_real, dm_fake}, ws,
                     ws_bytes, stream);
}

// ---- the same with the fused solve + sweep (kccot_sinkhorn_divergence_fused_f32) ----------------------------------
// forward = cost assembly -> ONE launch (three solves, combination, reverse sweep at dLoss = 1): C3 is scratch for the
// caller, dC3_unit [3,B,B] is what the backward needs; backward = coefficient build (x gloss) -> video gradient.
extern "C" int kccot_sinkhorn_loss_fused_fwd_f32(LOSS_INPUTS, float eps, int L, int Lmin, float thresh, unsigned flags,
                                                 float* C3, float* dC3_unit, float* cost3_out, int32_t* nits_out,
                                                 float* loss_out, int32_t* ticket, void* ws, size_t ws_bytes,
                                                 kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const LossCheck c{.inputs = false, .ptrs = C3 && dC3_unit && cost3_out && nits_out && loss_out && ticket,
                      .ws = WS_NULL_IF_EMPTY, .need = kccot_sinkhorn_loss_workspace_bytes(B, K)};
    if (int rc = loss_check("sinkhorn_loss_fused_fwd", a, c, ws, ws_bytes)) return rc;
    return loss3_fwd(false, a, Lmin, thresh, flags, C3, nullptr, nullptr, dC3_unit, cost3_out, nits_out, loss_out, ticket, ws,
                     ws_bytes, stream);
}

extern "C" int kccot_sinkhorn_loss_fused_bwd_f32(const float* gloss, const float* dC3_unit, LOSS_INPUTS, float* dfake,
                                                 float* dh_fake, float* dh_real, float* dm_real, float* dm_fake, void* ws,
                                                 size_t ws_bytes, kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, 0.f, 0};
    const LossCheck c{.inputs = false, .ptrs = gloss && dC3_unit, .ws = WS_UNCHECKED};      // the cost backward checks its own
    if (int rc = loss_check("sinkhorn_loss_fused_bwd", a, c, ws, ws_bytes)) return rc;
    return loss3_bwd(false, gloss, a, nullptr, nullptr, nullptr, nullptr, dC3_unit, {dfake, dh_fake, dh_real, dm_real, dm_fake},
                     ws, ws_bytes, stream);
}

// ---- the bi-causal loss (bicausal.hip) -------------------------------------------------------------------------------
extern "C" size_t kccot_bicausal_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    return kccot_sinkhorn_loss_workspace_bytes(B, K);      // the one-batch loss's layout
}

extern "C" int kccot_bicausal_sinkhorn_loss_fwd_f32(LOSS_INPUTS, float eps, int L, int Lmin, float thresh, unsigned flags,
                                                    float* C3, float* u_hist, float* v_hist, float* dC3_unit, float* cost3_out,
                                                    int32_t* nits_out, float* loss_out, int32_t* ticket, void* ws,
                                                    size_t ws_bytes, kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const LossCheck c{.inputs = true, .ptrs = C3 && cost3_out && nits_out && loss_out && ticket,
                      .hist = (u_hist == nullptr) == (v_hist == nullptr) && !(dC3_unit && u_hist),
                      .refused = flags & (KCCOT_COST_GRAM_SUMS_ONLY | KCCOT_COST_FROM_GRAM_SUMS), .ws = WS_REQUIRED,
                      .need = kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K)};
    if (int rc = loss_check("bicausal_sinkhorn_loss_fwd", a, c, ws, ws_bytes)) return rc;
    return loss3_fwd(true, a, Lmin, thresh, flags, C3, u_hist, v_hist, dC3_unit, cost3_out, nits_out, loss_out, ticket, ws,
                     ws_bytes, stream);
}

extern "C" int kccot_bicausal_sinkhorn_loss_bwd_f32(const float* gloss, LOSS_INPUTS, float eps, int L, const float* C3,
                                                    const float* u_hist, const float* v_hist, const int32_t* nits,
                                                    const float* dC3_unit, float* dfake, float* dh_fake, float* dh_real,
                                                    float* dm_real, float* dm_fake, void* ws, size_t ws_bytes,
                                                    kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const LossCheck c{.inputs = true, .ptrs = gloss != nullptr, .hist = dC3_unit || (C3 && u_hist && v_hist && nits),
                      .ws = WS_REQUIRED, .need = kccot_bicausal_sinkhorn_loss_workspace_bytes(B, K)};
    if (int rc = loss_check("bicausal_sinkhorn_loss_bwd", a, c, ws, ws_bytes)) return rc;
    return loss3_bwd(true, gloss, a, C3, u_hist, v_hist, nits, dC3_unit, {dfake, dh_fake, dh_real, dm_real, dm_fake}, ws,
                     ws_bytes, stream);
}

// ---- the one-batch loss with weighted marginals (include/kccot_weighted.h) -------------------------------------------
// 2 W(C_xy; a, b) - W(C_xx; a, a) - W(C_yy; b, b) with a = w_real, b = w_fake: the launch sequence of
// kccot_sinkhorn_loss_fwd_f32 / _bwd_f32 on the dual-history path with the weighted solver kernels.  An EXTENSION: the
// reference's compute_sinkhorn hard-codes uniform marginals.
extern "C" size_t kccot_weighted_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    return kccot_sinkhorn_loss_workspace_bytes(B, K);
}

extern "C" int kccot_weighted_sinkhorn_loss_fwd_f32(LOSS_INPUTS, float eps, int L, int Lmin, float thresh, unsigned flags,
                                                    const float* w_real, const float* w_fake, float* C3, float* u_hist,
                                                    float* v_hist, float* cost3_out, int32_t* nits_out, float* loss_out,
                                                    int32_t* ticket, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const LossCheck c{.inputs = true, .ptrs = w_real && w_fake && C3 && cost3_out && nits_out && loss_out && ticket,
                      .hist = (u_hist == nullptr) == (v_hist == nullptr), .ws = WS_REQUIRED,
                      .need = kccot_weighted_sinkhorn_loss_workspace_bytes(B, K)};
    if (int rc = loss_check("weighted_sinkhorn_loss_fwd", a, c, ws, ws_bytes)) return rc;
    return loss3_fwd(false, a, Lmin, thresh, flags, C3, u_hist, v_hist, nullptr, cost3_out, nits_out, loss_out, ticket, ws,
                     ws_bytes, stream, Weights{w_real, w_fake});
}

extern "C" int kccot_weighted_sinkhorn_loss_bwd_f32(const float* gloss, LOSS_INPUTS, float eps, int L, const float* w_real,
                                                    const float* w_fake, const float* C3, const float* u_hist,
                                                    const float* v_hist, const int32_t* nits, float* dfake, float* dh_fake,
                                                    float* dh_real, float* dm_real, float* dm_fake, void* ws, size_t ws_bytes,
                                                    kccot_stream_t stream) {
    return weighted_loss_bwd("weighted_sinkhorn_loss_bwd", gloss,
                             {real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L}, w_real, w_fake, C3, u_hist,
                             v_hist, nits, {dfake, dh_fake, dh_real, dm_real, dm_fake}, nullptr, nullptr, ws, ws_bytes, stream);
}

// ---- the same backward with the gradient w.r.t. the two weight vectors (include/kccot_weight_grad.h) --------------------
extern "C" size_t kccot_weighted_sinkhorn_loss_dw_workspace_bytes(int B, int64_t K) {
    const size_t base = kccot_weighted_sinkhorn_loss_workspace_bytes(B, K);
    return base ? base + weighted_dw_bytes(B) : 0;
}

extern "C" int kccot_weighted_sinkhorn_loss_bwd_dw_f32(const float* gloss, LOSS_INPUTS, float eps, int L, const float* w_real,
                                                       const float* w_fake, const float* C3, const float* u_hist,
                                                       const float* v_hist, const int32_t* nits, float* dfake, float* dh_fake,
                                                       float* dh_real, float* dm_real, float* dm_fake, float* dw_real,
                                                       float* dw_fake, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const char* who = "weighted_sinkhorn_loss_bwd_dw";
    if (!dw_real || !dw_fake) return fail(KCCOT_EINVAL, "%s: null dw_real / dw_fake", who);
    return weighted_loss_bwd(who, gloss, {real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L}, w_real, w_fake,
                             C3, u_hist, v_hist, nits, {dfake, dh_fake, dh_real, dm_real, dm_fake}, dw_real, dw_fake, ws,
                             ws_bytes, stream);
}

// ---- the kernel-conditional loss (include/kccot_conditional.h; its solver stage: conditional.hip) ------------------------
extern "C" size_t kccot_conditional_sinkhorn_loss_workspace_bytes(int B, int64_t K, int Q) {
    return cond_loss_ws_bytes(B, K, Q, false);
}

extern "C" int kccot_conditional_sinkhorn_loss_fwd_f32(LOSS_INPUTS, float eps, int L, int Lmin, float thresh, unsigned flags,
                                                       const float* w, const float* omega, int Q, float* C3, float* u_hist,
                                                       float* v_hist, float* cost_out, int32_t* nits_out, float* loss_out,
                                                       void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const LossArgs a{real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L};
    const unsigned refused =
        flags & (KCCOT_COST_BICAUSAL_TERM_ONLY | KCCOT_COST_RBF_SUM | KCCOT_COST_GRAM_SUMS_ONLY | KCCOT_COST_FROM_GRAM_SUMS);
    const LossCheck c{.inputs = true, .ptrs = w && C3 && cost_out && nits_out && loss_out,
                      .hist = (u_hist == nullptr) == (v_hist == nullptr), .refused = refused, .queries = &Q, .ws = WS_REQUIRED,
                      .need = cond_loss_ws_bytes(B, K, Q, false)};
    if (int rc = loss_check("conditional_sinkhorn_loss_fwd", a, c, ws, ws_bytes)) return rc;
    return loss3_fwd(false, a, Lmin, thresh, flags, C3, u_hist, v_hist, nullptr, cost_out, nits_out, loss_out, nullptr, ws,
                     ws_bytes, stream, Weights{w, omega, Q});
}

extern "C" int kccot_conditional_sinkhorn_loss_bwd_f32(const float* gloss, LOSS_INPUTS, float eps, int L, const float* w,
                                                       const float* omega, int Q, const float* C3, const float* u_hist,
                                                       const float* v_hist, const int32_t* nits, float* dfake, float* dh_fake,
                                                       float* dh_real, float* dm_real, float* dm_fake, void* ws,
                                                       size_t ws_bytes, kccot_stream_t stream) {
    return conditional_loss_bwd("conditional_sinkhorn_loss_bwd", gloss,
                                {real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L}, w, omega, Q, C3, u_hist,
                                v_hist, nits, {dfake, dh_fake, dh_real, dm_real, dm_fake}, nullptr, nullptr, nullptr, ws,
                                ws_bytes, stream);
}

// ---- the same backward with the gradients w.r.t. the weights (include/kccot_weight_grad.h) ------------------------------
extern "C" size_t kccot_conditional_sinkhorn_loss_dw_workspace_bytes(int B, int64_t K, int Q) {
    return cond_loss_ws_bytes(B, K, Q, true);
}

extern "C" int kccot_conditional_sinkhorn_loss_bwd_dw_f32(const float* gloss, LOSS_INPUTS, float eps, int L, const float* w,
                                                          const float* omega, int Q, const float* C3, const float* u_hist,
                                                          const float* v_hist, const int32_t* nits, float* dfake,
                                                          float* dh_fake, float* dh_real, float* dm_real, float* dm_fake,
                                                          const float* cost, float* dw_out, float* domega_out, void* ws,
                                                          size_t ws_bytes, kccot_stream_t stream) {
    const char* who = "conditional_sinkhorn_loss_bwd_dw";
    if (!cost || !dw_out) return fail(KCCOT_EINVAL, "%s: null cost / dw_out", who);
    return conditional_loss_bwd(who, gloss, {real, fake, B, K, sc, h_fake, h_real, m_real, m_fake, T, J, eps, L}, w, omega, Q,
                                C3, u_hist, v_hist, nits, {dfake, dh_fake, dh_real, dm_real, dm_fake}, cost, dw_out, domega_out,
                                ws, ws_bytes, stream);
}
