// Kernel-conditional Sinkhorn loss (include/kccot_conditional.h): Q weighted solves of the one-batch loss on ONE shared set
// of cost matrices, loss = sum_q omega_q (2 W(C_xy; w_q, w_q) - W(C_xx; w_q, w_q) - W(C_yy; w_q, w_q)).  An EXTENSION, not
// reference behaviour (the reference evaluates the loss with mu = nu = 1/n only).
//
// The solves are the weighted kernels of sinkhorn.hip / sinkhorn_gen.hip in their conditional mode (w_div = 2): problem
// p = 3 q + k reads cost matrix k of the shared C3 and weight row q, one workgroup per problem, so Q queries put 3 Q
// workgroups on the device where one loss call puts 3.  This file adds what surrounds them:
//   conditional_weights      the kernel estimator of the conditional law: a row softmax of -D / (2 bw^2) with a floor
//   conditional_combine_fwd  loss = sum_q omega_q (2 c_q0 - c_q1 - c_q2), double, ascending q
//   conditional_combine_bwd  gcost[3 q + k] = gloss omega_q {2,-1,-1}[k], on the device (no host round trip)
//   conditional_dC_reduce    dC3[k] = sum_q dC_{q,k}, double, ascending q, one thread per entry
//   conditional_dw_reduce    (kccot_weight_grad.h) dw[q] = sum_k (da_{3q+k} + db_{3q+k}), domega_q = gloss (2 c_q0 - c_q1 - c_q2)
//   conditional_weights_bwd  (kccot_weight_grad.h) the adjoint of conditional_weights from the stored weights
// and their host side: the solver stage cond_fwd / cond_bwd, which loss.hip sequences like its other stages, and the entry
// points of the solver-level pair and of the weight estimator.  Nothing here depends on the order in which workgroups finish:
// there is no atomic and no ticket.
#include "common.h"
#include <math.h>

namespace kccot {

constexpr int CD_MAXN = 1024;            // the streaming solver's limit
constexpr int CD_REG_MAXN = 128;         // register-resident kernels up to here (sinkhorn.hip: SK_MAXN)
constexpr int CD_MAXQ_STREAM = 21845;    // 3 Q problems in gridDim.z of the batched transposes
constexpr int CD_MAXQ = 1 << 24;         // 3 Q and 6 Q stay far inside an int
constexpr float CW_FLOOR = 0x1p-100f;    // a normal fp32 number; its log2 is exact
constexpr int CW_WAVES = 4;              // rows per workgroup of conditional_weights

// One wave per row q of D [Q,n]: w_qi = max(softmax_i(-D_qi / (2 bw^2)), 2^-100), scale2 = -log2(e) / (2 bw^2) <= 0.
// The shift is taken on the distances ((D_qi - min_i D_q.) scale2 is the shifted logit in log2 units, with ONE rounding of
// a difference instead of the difference of two rounded logits), the lanes stride over the row, exp2 is v_exp_f32.
// NaN propagates: a NaN distance gives a NaN sum and a row of NaN weights (the comparison with the floor keeps a NaN).
__device__ __forceinline__ void conditional_weights_rows(const float* __restrict__ D, int Q, int n, float scale2,
                                                         float* __restrict__ w) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * CW_WAVES + (threadIdx.x >> 6);
    if (row >= Q) return;                                   // wave-uniform
    const float* d = D + (int64_t)row * n;
    float* o = w + (int64_t)row * n;
    float mn = INFINITY;
    for (int j = lane; j < n; j += 64) mn = fminf(mn, d[j]);
    mn = -wave_max(-mn);
    double sd = 0.0;                                        // the sum in double: its only fp32 rounding is the final one
    for (int j = lane; j < n; j += 64) sd += (double)__builtin_amdgcn_exp2f((d[j] - mn) * scale2);
    const float s = (float)wave_sum_d(sd);                  // the same bits in every lane
    for (int j = lane; j < n; j += 64) {
        const float r = __builtin_amdgcn_exp2f((d[j] - mn) * scale2) / s;
        o[j] = r < CW_FLOOR ? CW_FLOOR : r;
    }
}
__global__ __launch_bounds__(CW_WAVES * 64) void conditional_weights(const float* __restrict__ D, int Q, int n, float scale2,
                                                                      float* __restrict__ w) {
    conditional_weights_rows(D, Q, n, scale2, w);
}

// scale2 of a bandwidth, in double (bandwidth^2 may leave the fp32 range: a huge bandwidth gives -0 and uniform weights); the
// host forms it with the same expression for the calls that take the bandwidth by value.  Not > 0: NaN.
__host__ __device__ inline float cw_scale2(float bandwidth) {
    if (!(bandwidth > 0.f)) return NAN;
    return (float)(-1.4426950408889634 / (2.0 * (double)bandwidth * (double)bandwidth));
}
// the same rows with the bandwidth read from device memory (kccot_conditional_weights_dev_f32)
__global__ __launch_bounds__(CW_WAVES * 64) void conditional_weights_dev(const float* __restrict__ D, int Q, int n,
                                                                          const float* __restrict__ bw,
                                                                          float* __restrict__ w) {
    conditional_weights_rows(D, Q, n, cw_scale2(bw[0]), w);
}

// Adjoint of conditional_weights, one wave per row, from the STORED weights: with l_qi = -D_qi / (2 bw^2) and s = softmax(l),
// w = max(s, floor); the floor has zero slope, so dl_qi = live ? w_qi (dw_qi - m_q) : 0 with m_q = sum_live w_qi dw_qi (the
// floored entries hold < 2^-100 of the softmax's mass), dD = -dl / (2 bw^2) and dbw_q = sum_i dl_qi D_qi / bw^3.  Sums and
// products in double.  `live` is !(w <= floor): a NaN weight is live and makes its row NaN.  bwp: the bandwidth in device
// memory, or null for the by-value `bw`.
__global__ __launch_bounds__(CW_WAVES * 64) void conditional_weights_bwd(const float* __restrict__ D, const float* __restrict__ w,
                                                                          const float* __restrict__ dw, int Q, int n, float bw,
                                                                          const float* __restrict__ bwp, float* __restrict__ dD,
                                                                          float* __restrict__ dbw) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * CW_WAVES + (threadIdx.x >> 6);
    if (row >= Q) return;                                   // wave-uniform
    if (bwp) bw = bwp[0];
    const double b = bw > 0.f ? (double)bw : (double)NAN;
    const float* d = D + (int64_t)row * n;
    const float* wr = w + (int64_t)row * n;
    const float* gr = dw + (int64_t)row * n;
    double m = 0.0;
    for (int j = lane; j < n; j += 64)
        if (!(wr[j] <= CW_FLOOR)) m += (double)wr[j] * (double)gr[j];
    m = wave_sum_d(m);
    const double inv2 = 1.0 / (2.0 * b * b);
    double sb = 0.0;
    for (int j = lane; j < n; j += 64) {
        const double dl = !(wr[j] <= CW_FLOOR) ? (double)wr[j] * ((double)gr[j] - m) : 0.0;
        dD[(int64_t)row * n + j] = (float)(-dl * inv2);
        sb += dl * (double)d[j];
    }
    sb = wave_sum_d(sb);
    if (lane == 0) dbw[row] = (float)(sb / (b * b * b));
}

__device__ __forceinline__ double query_weight(const float* omega, int q, int Q) {
    return omega ? (double)omega[q] : 1.0 / (double)Q;
}

// One wave: lane l forms the term of query base + l, then every lane adds the 64 terms in ascending q.
__global__ __launch_bounds__(64) void conditional_combine_fwd(const float* __restrict__ cost, const float* __restrict__ omega,
                                                              int Q, float* __restrict__ loss) {
    const int lane = threadIdx.x;
    double acc = 0.0;
    for (int base = 0; base < Q; base += 64) {
        const int q = base + lane;
        double term = 0.0;
        if (q < Q)
            term = query_weight(omega, q, Q) * ((2.0 * (double)cost[3 * q] - (double)cost[3 * q + 1]) - (double)cost[3 * q + 2]);
        const int cnt = Q - base < 64 ? Q - base : 64;
        for (int l = 0; l < cnt; ++l) acc += __shfl(term, l, 64);
    }
    if (lane == 0) loss[0] = (float)acc;
}

__global__ __launch_bounds__(256) void conditional_combine_bwd(const float* __restrict__ gloss, const float* __restrict__ omega,
                                                               int Q, float* __restrict__ gcost) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= 3 * Q) return;
    const int q = p / 3, k = p % 3;
    gcost[p] = (float)((double)gloss[0] * query_weight(omega, q, Q) * (k == 0 ? 2.0 : -1.0));
}

// dC3[k,i,j] = sum_q dCp[3 q + k, i, j]: entry e of dC3 [3 n n] is entry e of every query's block of 3 n n floats
__global__ __launch_bounds__(256) void conditional_dC_reduce(const float* __restrict__ dCp, int Q, int64_t n3,
                                                             float* __restrict__ dC3) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) acc += (double)dCp[(int64_t)q * n3 + e];
    dC3[e] = (float)acc;
}

// dw[q,i] = sum_k (da[3 q + k, i] + db[3 q + k, i]) (double, k = 0, 1, 2) from the per-problem weight gradients [3 Q,n], which
// carry gloss omega_q {2,-1,-1}[k] already; thread (q, 0) also writes domega[q] = gloss (2 c_q0 - c_q1 - c_q2) if wanted
__global__ __launch_bounds__(256) void conditional_dw_reduce(const float* __restrict__ da, const float* __restrict__ db,
                                                             const float* __restrict__ gloss, const float* __restrict__ cost,
                                                             int Q, int n, float* __restrict__ dw, float* __restrict__ domega) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (int64_t)Q * n) return;
    const int q = (int)(e / n), i = (int)(e % n);
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) acc += (double)da[(int64_t)(3 * q + k) * n + i] + (double)db[(int64_t)(3 * q + k) * n + i];
    dw[e] = (float)acc;
    if (domega && i == 0)
        domega[q] = (float)((double)gloss[0] * ((2.0 * (double)cost[3 * q] - (double)cost[3 * q + 1]) - (double)cost[3 * q + 2]));
}

// workspace of the solver-level pair: gcost [3 Q] | dCp [3 Q,n,n] | the streaming solver's stage (n > 128); the _dw backward
// (kccot_weight_grad.h) keeps the per-problem da | db [3 Q,n] each behind it, from `total` on
struct CondLayout { size_t off_dcp, off_gen, gen_bytes, total; };
static size_t cond_dadb_bytes(int Q, int n) { return up256((size_t)6 * Q * n * sizeof(float)); }
static CondLayout cond_layout(int Q, int n) {
    CondLayout l;
    l.off_dcp = up256((size_t)3 * Q * sizeof(float));
    l.off_gen = l.off_dcp + up256((size_t)3 * Q * n * n * sizeof(float));
    l.gen_bytes = n > CD_REG_MAXN ? sinkhorn_gen_conditional_workspace_bytes(Q, n) : 0;
    l.total = l.off_gen + l.gen_bytes;
    return l;
}

int cond_check(const char* who, int Q, int n, float eps, int L) {
    if (Q < 1 || n < 1 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "%s: bad arguments Q=%d n=%d L=%d eps=%g", who, Q, n, L, (double)eps);
    if (n > CD_MAXN) return fail(KCCOT_EUNSUPPORTED, "%s: n=%d > %d", who, n, CD_MAXN);
    if (Q > CD_MAXQ || (n > CD_REG_MAXN && Q > CD_MAXQ_STREAM))
        return fail(KCCOT_EUNSUPPORTED, "%s: Q=%d queries at n=%d (at most %d, %d on the streaming solver)", who, Q, n, CD_MAXQ,
                    CD_MAXQ_STREAM);
    return 0;
}

int cond_fwd(const float* C3, const float* w, const float* omega, int Q, int n, float eps, int L, int Lmin,
                    float thresh, float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out, float* loss_out, void* ws,
                    hipStream_t st) {
    const CondLayout l = cond_layout(Q, n);
    int rc = sinkhorn_conditional_solve_fwd(C3, w, Q, n, eps, L, Lmin, thresh, u_hist, v_hist, cost_out, nits_out,
                                            l.gen_bytes ? static_cast<char*>(ws) + l.off_gen : nullptr, l.gen_bytes, st);
    if (rc) return rc;
    hipLaunchKernelGGL(conditional_combine_fwd, dim3(1), dim3(64), 0, st, (const float*)cost_out, omega, Q, loss_out);
    return launch_status("conditional_combine_fwd");
}

// cost / dw_out / domega_out: the _dw backward (dw_out given: the workspace then extends by cond_dadb_bytes)
int cond_bwd(const float* gloss, const float* C3, const float* w, const float* omega, const float* u_hist,
                    const float* v_hist, const int32_t* nits, int Q, int n, float eps, int L, float* dC3_out, void* ws,
                    hipStream_t st, const float* cost, float* dw_out, float* domega_out) {
    const CondLayout l = cond_layout(Q, n);
    char* base = static_cast<char*>(ws);
    float* gcost = reinterpret_cast<float*>(base);
    float* dCp = reinterpret_cast<float*>(base + l.off_dcp);
    float* da = dw_out ? reinterpret_cast<float*>(base + l.total) : nullptr;
    float* db = dw_out ? da + (size_t)3 * Q * n : nullptr;
    hipLaunchKernelGGL(conditional_combine_bwd, dim3((3 * Q + 255) / 256), dim3(256), 0, st, gloss, omega, Q, gcost);
    int rc = launch_status("conditional_combine_bwd");
    if (rc) return rc;
    rc = sinkhorn_conditional_solve_bwd(C3, w, u_hist, v_hist, nits, Q, n, eps, L, gcost, dCp,
                                        l.gen_bytes ? base + l.off_gen : nullptr, l.gen_bytes, st, da, db);
    if (rc) return rc;
    const int64_t n3 = (int64_t)3 * n * n;
    hipLaunchKernelGGL(conditional_dC_reduce, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, st, (const float*)dCp, Q, n3,
                       dC3_out);
    if ((rc = launch_status("conditional_dC_reduce")) || !dw_out) return rc;
    const int64_t qn = (int64_t)Q * n;
    hipLaunchKernelGGL(conditional_dw_reduce, dim3((unsigned)((qn + 255) / 256)), dim3(256), 0, st, (const float*)da,
                       (const float*)db, gloss, cost, Q, n, dw_out, domega_out);
    return launch_status("conditional_dw_reduce");
}

}  // namespace kccot
using namespace kccot;

extern "C" int kccot_conditional_weights_f32(const float* D, int Q, int n, float bandwidth, float* w_out,
                                             kccot_stream_t stream) {
    if (!D || !w_out) return fail(KCCOT_EINVAL, "conditional_weights: null pointer");
    if (Q < 1 || n < 1) return fail(KCCOT_EINVAL, "conditional_weights: bad shape Q=%d n=%d", Q, n);
    if (!(bandwidth > 0.f)) return fail(KCCOT_EINVAL, "conditional_weights: bandwidth=%g is not > 0", (double)bandwidth);
    if (n > CD_MAXN) return fail(KCCOT_EUNSUPPORTED, "conditional_weights: n=%d > %d", n, CD_MAXN);
    const float scale2 = cw_scale2(bandwidth);
    hipLaunchKernelGGL(conditional_weights, dim3((Q + CW_WAVES - 1) / CW_WAVES), dim3(CW_WAVES * 64), 0, (hipStream_t)stream, D,
                       Q, n, scale2, w_out);
    return launch_status("conditional_weights");
}

extern "C" size_t kccot_sinkhorn_conditional_workspace_bytes(int Q, int n) {
    if (Q < 1 || n < 1 || n > CD_MAXN || Q > CD_MAXQ) return 0;
    return cond_layout(Q, n).total;
}

extern "C" int kccot_sinkhorn_conditional_fwd_f32(const float* C3, const float* w, const float* omega, int Q, int n, float eps,
                                                  int L, int Lmin, float thresh, float* u_hist, float* v_hist, float* cost_out,
                                                  int32_t* nits_out, float* loss_out, void* ws, size_t ws_bytes,
                                                  kccot_stream_t stream) {
    if (!C3 || !w || !cost_out || !nits_out || !loss_out) return fail(KCCOT_EINVAL, "sinkhorn_conditional_fwd: null pointer");
    if ((u_hist == nullptr) != (v_hist == nullptr))
        return fail(KCCOT_EINVAL, "sinkhorn_conditional_fwd: u_hist and v_hist must be given together");
    int rc = cond_check("sinkhorn_conditional_fwd", Q, n, eps, L);
    if (rc) return rc;
    const size_t need = cond_layout(Q, n).total;
    if (!ws || ws_bytes < need)
        return fail(KCCOT_EWORKSPACE, "sinkhorn_conditional_fwd: workspace %zu < %zu bytes", ws_bytes, need);
    return cond_fwd(C3, w, omega, Q, n, eps, L, Lmin, thresh, u_hist, v_hist, cost_out, nits_out, loss_out, ws,
                    (hipStream_t)stream);
}

extern "C" int kccot_sinkhorn_conditional_bwd_f32(const float* gloss, const float* C3, const float* w, const float* omega,
                                                  const float* u_hist, const float* v_hist, const int32_t* nits, int Q, int n,
                                                  float eps, int L, float* dC3_out, void* ws, size_t ws_bytes,
                                                  kccot_stream_t stream) {
    if (!gloss || !C3 || !w || !u_hist || !v_hist || !nits || !dC3_out)
        return fail(KCCOT_EINVAL, "sinkhorn_conditional_bwd: null pointer");
    int rc = cond_check("sinkhorn_conditional_bwd", Q, n, eps, L);
    if (rc) return rc;
    const size_t need = cond_layout(Q, n).total;
    if (!ws || ws_bytes < need)
        return fail(KCCOT_EWORKSPACE, "sinkhorn_conditional_bwd: workspace %zu < %zu bytes", ws_bytes, need);
    return cond_bwd(gloss, C3, w, omega, u_hist, v_hist, nits, Q, n, eps, L, dC3_out, ws, (hipStream_t)stream);
}

// ---- the gradients w.r.t. the weights (include/kccot_weight_grad.h) --------------------------------------------------------
extern "C" size_t kccot_sinkhorn_conditional_dw_workspace_bytes(int Q, int n) {
    if (Q < 1 || n < 1 || n > CD_MAXN || Q > CD_MAXQ) return 0;
    return cond_layout(Q, n).total + cond_dadb_bytes(Q, n);
}

extern "C" int kccot_sinkhorn_conditional_bwd_dw_f32(const float* gloss, const float* C3, const float* w, const float* omega,
                                                     const float* u_hist, const float* v_hist, const int32_t* nits, int Q,
                                                     int n, float eps, int L, float* dC3_out, const float* cost,
                                                     float* dw_out, float* domega_out, void* ws, size_t ws_bytes,
                                                     kccot_stream_t stream) {
    const char* who = "sinkhorn_conditional_bwd_dw";
    if (!gloss || !C3 || !w || !u_hist || !v_hist || !nits || !dC3_out || !cost || !dw_out)
        return fail(KCCOT_EINVAL, "%s: null pointer", who);
    int rc = cond_check(who, Q, n, eps, L);
    if (rc) return rc;
    const size_t need = kccot_sinkhorn_conditional_dw_workspace_bytes(Q, n);
    if (!ws || ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return cond_bwd(gloss, C3, w, omega, u_hist, v_hist, nits, Q, n, eps, L, dC3_out, ws, (hipStream_t)stream, cost, dw_out,
                    domega_out);
}

static int cw_bwd_check(const char* who, const void* D, const void* w, const void* dw, int Q, int n, const void* dD,
                        const void* dbw) {
    if (!D || !w || !dw || !dD || !dbw) return fail(KCCOT_EINVAL, "%s: null pointer", who);
    if (Q < 1 || n < 1) return fail(KCCOT_EINVAL, "%s: bad shape Q=%d n=%d", who, Q, n);
    if (n > CD_MAXN) return fail(KCCOT_EUNSUPPORTED, "%s: n=%d > %d", who, n, CD_MAXN);
    return 0;
}

extern "C" int kccot_conditional_weights_bwd_f32(const float* D, const float* w, const float* dw, int Q, int n,
                                                 float bandwidth, float* dD_out, float* dbw_out, kccot_stream_t stream) {
    const char* who = "conditional_weights_bwd";
    int rc = cw_bwd_check(who, D, w, dw, Q, n, dD_out, dbw_out);
    if (rc) return rc;
    if (!(bandwidth > 0.f)) return fail(KCCOT_EINVAL, "%s: bandwidth=%g is not > 0", who, (double)bandwidth);
    hipLaunchKernelGGL(conditional_weights_bwd, dim3((Q + CW_WAVES - 1) / CW_WAVES), dim3(CW_WAVES * 64), 0,
                       (hipStream_t)stream, D, w, dw, Q, n, bandwidth, (const float*)nullptr, dD_out, dbw_out);
    return launch_status(who);
}

extern "C" int kccot_conditional_weights_bwd_dev_f32(const float* D, const float* w, const float* dw, int Q, int n,
                                                     const float* bandwidth, float* dD_out, float* dbw_out,
                                                     kccot_stream_t stream) {
    const char* who = "conditional_weights_bwd_dev";
    int rc = cw_bwd_check(who, D, w, dw, Q, n, dD_out, dbw_out);
    if (rc) return rc;
    if (!bandwidth) return fail(KCCOT_EINVAL, "%s: null bandwidth pointer", who);
    hipLaunchKernelGGL(conditional_weights_bwd, dim3((Q + CW_WAVES - 1) / CW_WAVES), dim3(CW_WAVES * 64), 0,
                       (hipStream_t)stream, D, w, dw, Q, n, 0.f, bandwidth, dD_out, dbw_out);
    return launch_status(who);
}

extern "C" int kccot_conditional_weights_dev_f32(const float* D, int Q, int n, const float* bandwidth, float* w_out,
                                                 kccot_stream_t stream) {
    if (!D || !w_out || !bandwidth) return fail(KCCOT_EINVAL, "conditional_weights_dev: null pointer");
    if (Q < 1 || n < 1) return fail(KCCOT_EINVAL, "conditional_weights_dev: bad shape Q=%d n=%d", Q, n);
    if (n > CD_MAXN) return fail(KCCOT_EUNSUPPORTED, "conditional_weights_dev: n=%d > %d", n, CD_MAXN);
    hipLaunchKernelGGL(conditional_weights_dev, dim3((Q + CW_WAVES - 1) / CW_WAVES), dim3(CW_WAVES * 64), 0,
                       (hipStream_t)stream, D, Q, n, bandwidth, w_out);
    return launch_status("conditional_weights_dev");
}
