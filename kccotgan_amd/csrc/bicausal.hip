// Bi-causal Sinkhorn loss (an extension: the reference ships bi_causal_modified_cost, gan_utils.py:46-72, and
// compute_sinkhorn(..., bi_causal=True), gan_utils.py:124-136, and names the mode in kernel_train.py's --bi_causal flag,
// :396, but its compute_sinkhorn_loss never passes bi_causal):
//
//   loss = 2 W(x,y) - W(x,x) - W(y,y),   W = compute_sinkhorn(..., bi_causal=True)
//   W(x,y) = compute_sinkhorn(real, fake, h_fake, m_real, sc, hx=h_real, My=m_fake, bi_causal=True)
//   W(x,x) = compute_sinkhorn(real, real, h_real, m_real, sc, hx=h_real, My=m_real, bi_causal=True)
//   W(y,y) = compute_sinkhorn(fake, fake, h_fake, m_fake, sc, hx=h_fake, My=m_fake, bi_causal=True)
//
// With causal(h, M)[i,j] = sc sum_{t<T-1,q} h[i,t,q] (M[j,t+1,q] - M[j,t,q])  (h indexes rows, M columns):
//   C_xy = sc |x_i - y_j|^2 + causal(h_fake, m_real) + causal(h_real, m_fake)
//   C_xx = sc |x_i - x_j|^2 + causal(h_real, m_real) + causal(h_real, m_real)     (the same fp32 term twice)
//   C_yy = sc |y_i - y_j|^2 + causal(h_fake, m_fake) + causal(h_fake, m_fake)
// The first causal term of each matrix is exactly the one-batch loss's, so
//   forward : kccot_pairwise_cost3_f32 (the one-batch C3, any rung of the cost ladder) -> bicausal_cost_add (the second
//             term of each matrix added in place) -> the three solves + combination (fused solve + sweep, or history)
//   backward: [history path: reverse sweep] -> the one-batch cost backward with the bi-causal feature-gradient job table
//             (cost_bwd.hip: per-term weights 1, 2); dfake is the one-batch loss's (the distance part is unchanged).
// The entry points kccot_bicausal_sinkhorn_loss_* run the one-batch loss's host sequence (loss.hip) with these two changes.
#include "common.h"

namespace kccot {

struct BicausalAdd {
    const float* h[3];    // rows:    h_real (xy), h_real (xx), h_fake (yy)
    const float* M[3];    // columns: m_fake (xy), m_real (xx), m_fake (yy)
};

// C3[p] += causal(h[p], M[p]) on 8 x 8 output tiles (blockIdx.z = problem): 192 workgroups at B = 64, so that the
// latency-bound load and the LDS reads are spread over most of the CUs.  A k chunk of BC_KC = 256 values ((T-1) J = 232 at
// T = 30, J = 8: one chunk) of the eight h rows and the eight first differences of the M rows is staged through LDS with all
// 24 loads of a thread in flight; the four waves then take one quarter of the chunk each for the 64 outputs, and the
// quarters are added in a fixed order.  (The first form, causal_tile16 on 16 x 16 tiles: 48 workgroups, 48 spilled SGPRs
// for the sixteen row bases per operand, 10.3 us at configs[1].)
constexpr int BC_TILE = 8;
constexpr int BC_KC = 256;
constexpr int BC_PITCH = BC_KC + 4;   // rows 4 banks apart: the eight column rows of a wave's float4 reads are conflict-free

__global__ __launch_bounds__(256) void bicausal_cost_add(float* __restrict__ C3, BicausalAdd a, int B, int T, int J,
                                                         float sc) {
    __shared__ __attribute__((aligned(16))) float sh[BC_TILE * BC_PITCH];
    __shared__ __attribute__((aligned(16))) float sm[BC_TILE * BC_PITCH];
    __shared__ float part[4 * 64];
    const int p = blockIdx.z, i0 = blockIdx.y * BC_TILE, j0 = blockIdx.x * BC_TILE;
    const int t = threadIdx.x, o = t & 63, q = t >> 6, oi = o >> 3, oj = o & 7;
    const int KK = (T - 1) * J, TJ = T * J;
    const float* __restrict__ h = a.h[p];
    const float* __restrict__ M = a.M[p];
    float acc = 0.f;
    for (int k0 = 0; k0 < KK; k0 += BC_KC) {
        // addresses clamped into range (rows to B-1, k to 0): the loads carry no control dependence; zeros selected below
        const int k = k0 + t;
        const bool kok = k < KK;
        const int kc = kok ? k : 0;
        float hv[BC_TILE], m0[BC_TILE], m1[BC_TILE];
#pragma unroll
        for (int r = 0; r < BC_TILE; ++r) {
            const int ri = (i0 + r < B) ? i0 + r : B - 1, rj = (j0 + r < B) ? j0 + r : B - 1;
            hv[r] = h[(int64_t)ri * TJ + kc];
            const float* mr = M + (int64_t)rj * TJ + kc;
            m0[r] = mr[0];
            m1[r] = mr[J];
        }
#pragma unroll
        for (int r = 0; r < BC_TILE; ++r) {
            sh[r * BC_PITCH + t] = (kok && i0 + r < B) ? hv[r] : 0.f;
            sm[r * BC_PITCH + t] = (kok && j0 + r < B) ? m1[r] - m0[r] : 0.f;
        }
        __syncthreads();
        const float* hr = sh + oi * BC_PITCH + q * 64;
        const float* mr = sm + oj * BC_PITCH + q * 64;
        float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
#pragma unroll
        for (int kk = 0; kk < 64; kk += 4) {
            const float4 x = *reinterpret_cast<const float4*>(hr + kk);
            const float4 y = *reinterpret_cast<const float4*>(mr + kk);
            t0 = fmaf(x.x, y.x, t0); t1 = fmaf(x.y, y.y, t1); t2 = fmaf(x.z, y.z, t2); t3 = fmaf(x.w, y.w, t3);
        }
        acc += (t0 + t1) + (t2 + t3);
        __syncthreads();
    }
    part[q * 64 + o] = acc;
    __syncthreads();
    if (t < 64) {
        const int i = i0 + oi, j = j0 + oj;
        if (i < B && j < B) {
            float* c = C3 + ((int64_t)p * B + i) * B + j;
            *c += ((part[o] + part[64 + o]) + (part[128 + o] + part[192 + o])) * sc;
        }
    }
}

int launch_bicausal_cost_add(float* C3, int B, const float* h_fake, const float* h_real, const float* m_real,
                             const float* m_fake, int T, int J, float sc, hipStream_t st) {
    const unsigned tiles = (unsigned)((B + BC_TILE - 1) / BC_TILE);
    hipLaunchKernelGGL(bicausal_cost_add, dim3(tiles, tiles, 3), dim3(256), 0, st, C3,
                       BicausalAdd{{h_real, h_real, h_fake}, {m_fake, m_real, m_fake}}, B, T, J, sc);
    return launch_status("bicausal_cost_add");
}

}  // namespace kccot
