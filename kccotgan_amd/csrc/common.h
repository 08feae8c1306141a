// Shared host/device helpers for the kccot HIP kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include "../../include/kccot.h"
#include "../../include/kccot_weighted.h"
#include "../../include/kccot_conditional.h"
#include "../../include/kccot_weight_grad.h"

#define KCCOT_WAVE 64

namespace kccot {

void set_error(const char* fmt, ...);

inline int fail(int code, const char* fmt, ...) {
    char buf[384];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error("%s", buf);
    return code;
}

inline int launch_status(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
inline size_t max3(size_t a, size_t b, size_t c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }

// ---- wave-level reductions (64-wide wavefront; xor butterflies leave the result in every lane)
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also drains the vector-memory
// counter (vmcnt(0)), which would put every outstanding global store / prefetch load on the critical
// path of a loop that synchronises through LDS alone; LDS visibility needs lgkmcnt(0) + s_barrier.
__device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// ---- DPP reductions inside aligned groups of LPR <= 16 lanes; every lane gets the result -----
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}
// max(v, dpp(v)) in ONE instruction.  fmaxf() on a DPP move costs mov + canonicalise + max; the
// values here are never NaN-signalling, so the bare v_max_f32_dpp is exact.  The s_nop covers the
// VALU-write -> DPP-read hazard (2 wait states) that hipcc does not pad inside an asm statement.
#define KCCOT_DPP_MAX(V, CTRL)                                                                          \
    asm volatile("s_nop 1\n\tv_max_f32_dpp %0, %1, %1 " CTRL " row_mask:0xf bank_mask:0xf" : "=v"(V) : "v"(V))
template <int LPR>
__device__ __forceinline__ float seg_max(float v) {
    if (LPR >= 2) KCCOT_DPP_MAX(v, "quad_perm:[1,0,3,2]");
    if (LPR >= 4) KCCOT_DPP_MAX(v, "quad_perm:[2,3,0,1]");
    if (LPR >= 8) KCCOT_DPP_MAX(v, "row_half_mirror");
    if (LPR >= 16) KCCOT_DPP_MAX(v, "row_mirror");
    return v;
}
template <int LPR>
__device__ __forceinline__ float seg_sum(float v) {
    if (LPR >= 2) v += dpp_mov<0xB1>(v);
    if (LPR >= 4) v += dpp_mov<0x4E>(v);
    if (LPR >= 8) v += dpp_mov<0x141>(v);
    if (LPR >= 16) v += dpp_mov<0x140>(v);
    return v;
}

// DPP forms for latency-critical loops: four in-row steps (every lane of a 16-lane row ends with its row's
// result), then the four row results are read through SGPRs.  ~11 instructions and no LDS-crossbar round
// trips (a __shfl_xor butterfly is six dependent ds_bpermute_b32).  The result is wave-uniform.
__device__ __forceinline__ float wave_row_dpp_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));  // row_mirror
    return v;
}
__device__ __forceinline__ float wave_sum_fast(float v) {
    v = wave_row_dpp_sum(v);
    const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return (a + b) + (c + d);
}
__device__ __forceinline__ float wave_max_fast(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false)));
    const float a = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float b = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float d = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return fmaxf(fmaxf(a, b), fmaxf(c, d));
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Block-wide sum with a fixed (deterministic) combination order.  `scratch` holds >= 16 floats
// of LDS.  Every thread of the block must call it; every thread receives the result.
__device__ __forceinline__ float block_sum(float v, float* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float r = 0.f;
    for (int w = 0; w < nw; ++w) r += scratch[w];
    return r;
}
__device__ __forceinline__ float block_max(float v, float* scratch) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) scratch[wid] = v;
    __syncthreads();
    float r = scratch[0];
    for (int w = 1; w < nw; ++w) r = fmaxf(r, scratch[w]);
    return r;
}

// sinkhorn.hip: `nprob` (3 or 4) fused solves + weighted combination + reverse sweep in one launch (sinkhorn_fused_reg);
// loss_out = sum_p w[p] cost[p], dC_unit = d loss / d C at dLoss = 1.  Eligibility: kccot_sinkhorn_fused_eligible(n, L).
int sinkhorn_fused_weighted(const float* C, int nprob, const float* w, int n, float eps, int L, int Lmin, float thresh,
                            float* cost_out, int32_t* nits_out, float* loss_out, int32_t* ticket, float* dC_unit,
                            hipStream_t st);

// sinkhorn.hip: the divergence with weighted marginals (a,b), (a,a), (b,b) on C3 = [xy, xx, yy]; a = w_real, b = w_fake [n]
int sinkhorn_divergence_weighted_fwd(const float* C3, const float* w_real, const float* w_fake, int n, float eps, int L,
                                     int Lmin, float thresh, float* u_hist, float* v_hist, float* cost3_out,
                                     int32_t* nits_out, float* loss_out, int32_t* ticket, void* ws, size_t ws_bytes,
                                     hipStream_t st);
int sinkhorn_divergence_weighted_bwd(const float* C3, const float* w_real, const float* w_fake, const float* u_hist,
                                     const float* v_hist, const int32_t* nits, int n, float eps, int L, const float* gloss,
                                     float* gc3, float* dC3, void* ws, size_t ws_bytes, hipStream_t st,
                                     float* da3 = nullptr, float* db3 = nullptr);

// sinkhorn.hip: the 3 Q solves / reverse sweeps of the conditional loss (kccot_conditional.h) on ONE shared C3 [3,n,n]:
// problem p = 3 q + k reads cost matrix k and weight row q of w [Q,n]; histories, costs, counts, gcost [3 Q] and dC
// [3 Q,n,n] are indexed by p.  ws (n > 128 only): sinkhorn_gen_conditional_workspace_bytes(Q, n) bytes (sinkhorn_gen.hip).
size_t sinkhorn_gen_conditional_workspace_bytes(int Q, int n);
int sinkhorn_conditional_solve_fwd(const float* C3, const float* w, int Q, int n, float eps, int L, int Lmin, float thresh,
                                   float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out, void* ws,
                                   size_t ws_bytes, hipStream_t st);
int sinkhorn_conditional_solve_bwd(const float* C3, const float* w, const float* u_hist, const float* v_hist,
                                   const int32_t* nits, int Q, int n, float eps, int L, const float* gcost, float* dC,
                                   void* ws, size_t ws_bytes, hipStream_t st, float* da = nullptr, float* db = nullptr);

// conditional.hip: the solver stage of the conditional loss on a finished C3 [3,n,n], after cond_check (its limits on Q and n:
// KCCOT_EINVAL / KCCOT_EUNSUPPORTED).  cond_fwd: the 3 Q solves -> loss = sum_q omega_q (2 c_q0 - c_q1 - c_q2); cond_bwd: gcost ->
// the 3 Q reverse sweeps -> dC3_out = sum_q dC_q [-> dw_out [Q,n], domega_out [Q] (may be null) from the forward's cost [Q,3]].
// ws: kccot_sinkhorn_conditional_workspace_bytes(Q, n) bytes, with dw_out kccot_sinkhorn_conditional_dw_workspace_bytes(Q, n).
int cond_check(const char* who, int Q, int n, float eps, int L);
int cond_fwd(const float* C3, const float* w, const float* omega, int Q, int n, float eps, int L, int Lmin, float thresh,
             float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out, float* loss_out, void* ws, hipStream_t st);
int cond_bwd(const float* gloss, const float* C3, const float* w, const float* omega, const float* u_hist, const float* v_hist,
             const int32_t* nits, int Q, int n, float eps, int L, float* dC3_out, void* ws, hipStream_t st,
             const float* cost = nullptr, float* dw_out = nullptr, float* domega_out = nullptr);

// cost_bwd.hip: kccot_pairwise_cost3_bwd_scaled_f32 (gscale = NULL: unscaled) over the whole batch.  bicausal selects the
// feature-gradient jobs of the bi-causal loss (bicausal.hip): dh_fake = gxy.dm_real + 2 gyy.dm_fake,
// dh_real = gxy.dm_fake + 2 gxx.dm_real, dm_real = gxy with h_fake + 2 gxx with h_real, dm_fake = gxy with h_real +
// 2 gyy with h_fake; dfake as the one-batch loss.
int cost3_bwd_loss(const float* g3, const float* gscale, const float* real, const float* fake, int B, int64_t K, float sc,
                   const float* h_fake, const float* h_real, const float* m_real, const float* m_fake, int T, int J,
                   float* dfake, float* dh_fake, float* dh_real, float* dm_real, float* dm_fake, void* ws, size_t ws_bytes,
                   hipStream_t st, bool bicausal);

// bicausal.hip: C3 [3,B,B] += the second causal term of each bi-causal cost matrix, in place
int launch_bicausal_cost_add(float* C3, int B, const float* h_fake, const float* h_real, const float* m_real,
                             const float* m_fake, int T, int J, float sc, hipStream_t st);

// mixed.hip: C [Bx,By] += sc causal(h, M) in place, summed as mixed_cost_finalize sums it (KCCOT_COST_CAUSAL_ADD)
int launch_mixed_causal_add(float* C, int Bx, int By, const float* h, const float* M, int T, int J, float sc,
                            hipStream_t st);

// rbf_sum.hip: C [Bx,By] = exp(-gamma C) in place, the fp64 sum of the block at ws[0] (KCCOT_COST_RBF_SUM); the call
// touches the first rbf_sum_doubles(Bx, By) doubles of ws (the sum, then one partial per 4 x 64 tile)
size_t rbf_sum_doubles(int Bx, int By);
int launch_rbf_sum(float* C, int Bx, int By, float gamma, double* ws, hipStream_t st);

}  // namespace kccot
