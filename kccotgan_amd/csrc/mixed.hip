// Mixed Sinkhorn divergence over two minibatches (COT-GAN's estimator; an extension: the reference's
// compute_sinkhorn_loss, gan_utils.py:204-227, describes x, x' and y, y' in its docstring but evaluates the one-batch form):
//
//   loss = (W(x,y) + W(x',y')) - W(x,x') - W(y,y'),   W = compute_sinkhorn (gan_utils.py:124, bi_causal = False)
//
//   term  cost matrix                      rows h     cols M
//   C1    sc |x_i  - y_j |^2 + causal      h_fake     m_real
//   C2    sc |x'_i - y'_j|^2 + causal      h_fake_p   m_real_p
//   C3    sc |x_i  - x'_j|^2 + causal      h_real_p   m_real
//   C4    sc |y_i  - y'_j|^2 + causal      h_fake_p   m_fake
//
// The squared distances come from ONE kccot_pairwise_cost3_f32 call on the stacked minibatches R = [x; x'], F = [y; y']
// ([2B,K] each; plain scaled distances D3 = [RF, RR, FF], each [2B,2B]); C1..C4 are blocks of it:
//   C1 = RF[0:B,0:B], C2 = RF[B:,B:], C3 = RR[0:B,B:], C4 = FF[0:B,B:].
// That computes 12 B^2 distances of which 4 B^2 are used (about 3x the matrix-pipe work of a dedicated four-block
// kernel, for the same HBM bytes: every video is read once) -- DESIGN.md section 10.
//
// This file adds the two small kernels around the existing stages and sequences them:
//   forward : cost3(R, F) -> mixed_cost_finalize (blocks + causal terms -> Cmix [4,B,B]) ->
//             four solves + combination (+ reverse sweep at dLoss = 1 when fused)
//   backward: [history path: gcost = gloss w -> reverse sweep] -> mixed_cost_bwd (g3 [3,2B,2B] of the stacked problem
//             + the six feature gradients) -> cost3 backward (d[y; y'] as one [2B,K] tensor)
#include "common.h"

namespace kccot {

static const float kMixW[4] = {1.0f, 1.0f, -1.0f, -1.0f};   // (W1 + W2) - W3 - W4

struct MixFeats {
    const float* h[4];    // row features of C1..C4:    h_fake, h_fake_p, h_real_p, h_fake_p
    const float* M[4];    // column features of C1..C4: m_real, m_real_p, m_real, m_fake
};

// Cmix[k,i,j] = D3 block of term k + sc * sum_{t<T-1,q} h_k[i,t,q] (M_k[j,t+1,q] - M_k[j,t,q])   (gan_utils.py:33-38)
// One thread per entry; the causal contraction ((T-1) J terms, fp32 differences as the reference forms them) is
// accumulated in fp64 and added once.
__global__ __launch_bounds__(256) void mixed_cost_finalize(const float* __restrict__ D3, MixFeats f, int B, int T, int J,
                                                           float sc, float* __restrict__ Cmix) {
    const int64_t bb = (int64_t)B * B, n2 = 2 * (int64_t)B;
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= 4 * bb) return;
    const int k = (int)(e / bb), i = (int)((e / B) % B), j = (int)(e % B);
    // (matrix of D3, row offset, column offset) of the block
    const int mat = k < 2 ? 0 : k - 1;
    const int r0 = k == 1 ? B : 0, c0 = B * (k != 0);
    const float d = D3[mat * n2 * n2 + (int64_t)(r0 + i) * n2 + (c0 + j)];
    const int TJ = T * J;
    const float* h = f.h[k] + (int64_t)i * TJ;
    const float* M = f.M[k] + (int64_t)j * TJ;
    double acc = 0.0;
    for (int x = 0; x < (T - 1) * J; ++x) acc += (double)h[x] * (double)(M[x + J] - M[x]);
    Cmix[e] = d + (float)(acc * (double)sc);
}

// KCCOT_COST_CAUSAL_ADD (kccot_pairwise_cost_f32): C[i,j] += sc causal(h, M)[i,j] on a finished block, for a caller that
// assembles Cmix from row blocks of the stacked problem (kccotgan_amd/dist.py, the batch-sharded mixed loss).  Each entry
// is summed exactly as mixed_cost_finalize sums it -- the fp32 first difference of M, then (double)h * (double)dM
// accumulated in fp64 in ascending term order, then ONE (float)(acc * sc) added to C -- so that, given equal distances,
// the entries equal the single-GPU Cmix bit for bit.  16 x 16 output tiles; a k chunk of CA_KC terms of the 16 h rows and
// of the 16 first differences of the M rows is staged through LDS (the pattern of causal_tile16, cost_internal.h), all
// 48 loads of a thread in flight before the one wait; each thread then walks its row and column in order.
constexpr int CA_TILE = 16;
constexpr int CA_KC = 256;
constexpr int CA_PITCH = CA_KC + 4;   // rows 16-byte aligned and 4 banks apart: conflict-free float4 reads

__global__ __launch_bounds__(256) void mixed_causal_add(float* __restrict__ C, const float* __restrict__ h,
                                                        const float* __restrict__ M, int Bx, int By, int T, int J, float sc) {
    __shared__ __attribute__((aligned(16))) float sh[CA_TILE * CA_PITCH];
    __shared__ __attribute__((aligned(16))) float sm[CA_TILE * CA_PITCH];
    const int i0 = blockIdx.y * CA_TILE, j0 = blockIdx.x * CA_TILE;
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const int KK = (T - 1) * J, TJ = T * J;
    double acc = 0.0;
    for (int k0 = 0; k0 < KK; k0 += CA_KC) {
        // addresses clamped into range (rows to the last one, k to 0): no control dependence on the loads; the selects
        // below write zeros for the lanes out of range, and a zero term leaves the fp64 sum unchanged
        const int k = k0 + t;
        const bool kok = k < KK;
        const int kc = kok ? k : 0;
        float hv[CA_TILE], m0[CA_TILE], m1[CA_TILE];
#pragma unroll
        for (int r = 0; r < CA_TILE; ++r) {
            const int ri = (i0 + r < Bx) ? i0 + r : Bx - 1, rj = (j0 + r < By) ? j0 + r : By - 1;
            hv[r] = h[(int64_t)ri * TJ + kc];
            const float* mr = M + (int64_t)rj * TJ + kc;
            m0[r] = mr[0];
            m1[r] = mr[J];
        }
#pragma unroll
        for (int r = 0; r < CA_TILE; ++r) {
            sh[r * CA_PITCH + t] = (kok && i0 + r < Bx) ? hv[r] : 0.f;
            sm[r * CA_PITCH + t] = (kok && j0 + r < By) ? m1[r] - m0[r] : 0.f;
        }
        __syncthreads();
        const int n = KK - k0 < CA_KC ? KK - k0 : CA_KC;
        const float* hr = sh + ti * CA_PITCH;
        const float* mr = sm + tj * CA_PITCH;
#pragma unroll 8
        for (int kk = 0; kk < n; kk += 4) {
            const float4 a = *reinterpret_cast<const float4*>(hr + kk);
            const float4 b = *reinterpret_cast<const float4*>(mr + kk);
            // the expression of mixed_cost_finalize, term by term
            acc += (double)a.x * (double)b.x;
            acc += (double)a.y * (double)b.y;
            acc += (double)a.z * (double)b.z;
            acc += (double)a.w * (double)b.w;
        }
        __syncthreads();
    }
    const int i = i0 + ti, j = j0 + tj;
    if (i < Bx && j < By) {
        float* c = C + (int64_t)i * By + j;
        *c = *c + (float)(acc * (double)sc);
    }
}

int launch_mixed_causal_add(float* C, int Bx, int By, const float* h, const float* M, int T, int J, float sc,
                            hipStream_t st) {
    hipLaunchKernelGGL(mixed_causal_add, dim3((unsigned)((By + CA_TILE - 1) / CA_TILE), (unsigned)((Bx + CA_TILE - 1) / CA_TILE)),
                       dim3(256), 0, st, C, h, M, Bx, By, T, J, sc);
    return launch_status("mixed_causal_add");
}

struct MixBwdArgs {
    const float* dC;      // [4,B,B] d loss / d Cmix (at dLoss = 1 when gscale != NULL)
    const float* gscale;  // ONE device float or NULL (= 1)
    MixFeats f;
    float* g3;            // [3,2B,2B] coefficients of the stacked problem
    float* dfeat[6];      // h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p (each may be NULL)
    int B, T, J;
    float sc;
};

// d causal / d h[i,t,q] = sc sum_j dC[i,j] (M[j,t+1,q] - M[j,t,q])            (t < T-1; 0 at t = T-1)
__device__ __forceinline__ float mix_dh(const float* __restrict__ dC, const float* __restrict__ M, int B, int T, int J,
                                        int i, int t, int q) {
    if (t >= T - 1) return 0.f;
    const int TJ = T * J;
    const float* g = dC + (int64_t)i * B;
    float s = 0.f;
    for (int j = 0; j < B; ++j) {
        const float* m = M + (int64_t)j * TJ + t * J + q;
        s += g[j] * (m[J] - m[0]);
    }
    return s;
}

// d causal / d M[j,t,q] = sc sum_i dC[i,j] (h[i,t-1,q] [t >= 1] - h[i,t,q] [t < T-1])
__device__ __forceinline__ float mix_dM(const float* __restrict__ dC, const float* __restrict__ h, int B, int T, int J,
                                        int j, int t, int q) {
    const int TJ = T * J;
    float s = 0.f;
    for (int i = 0; i < B; ++i) {
        const float* hh = h + (int64_t)i * TJ + t * J + q;
        const float w = (t >= 1 ? hh[-J] : 0.f) - (t < T - 1 ? hh[0] : 0.f);
        s += dC[(int64_t)i * B + j] * w;
    }
    return s;
}

// One launch: the g3 coefficients (dC1 -> RF block (0,0), dC2 -> RF block (1,1), dC4 -> FF block (0,1), zeros elsewhere;
// dC3 reaches the features only: real videos get no gradient) and the six feature gradients
// (h_fake_p from C2 and C4, m_real from C1 and C3).
__global__ __launch_bounds__(256) void mixed_cost_bwd(MixBwdArgs a) {
    const int B = a.B, T = a.T, J = a.J;
    const int64_t bb = (int64_t)B * B, n2 = 2 * (int64_t)B, ng3 = 3 * n2 * n2, nf = (int64_t)B * T * J;
    const float gs = a.gscale ? a.gscale[0] : 1.0f;
    const int64_t total = ng3 + 6 * nf;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        if (e < ng3) {
            const int mat = (int)(e / (n2 * n2));
            const int r = (int)((e / n2) % n2), c = (int)(e % n2);
            const bool rlo = r < B, clo = c < B;
            float v = 0.f;
            if (mat == 0 && rlo && clo) v = a.dC[(int64_t)r * B + c];                              // C1
            else if (mat == 0 && !rlo && !clo) v = a.dC[bb + (int64_t)(r - B) * B + (c - B)];      // C2
            else if (mat == 2 && rlo && !clo) v = a.dC[3 * bb + (int64_t)r * B + (c - B)];         // C4
            a.g3[e] = v * gs;
            continue;
        }
        const int64_t x = e - ng3;
        const int o = (int)(x / nf);
        float* out = a.dfeat[o];
        if (!out) continue;
        const int64_t y = x % nf;
        const int b = (int)(y / (T * J)), t = (int)((y / J) % T), q = (int)(y % J);
        const float* dC1 = a.dC;
        const float* dC2 = a.dC + bb;
        const float* dC3 = a.dC + 2 * bb;
        const float* dC4 = a.dC + 3 * bb;
        float s;
        switch (o) {
            case 0: s = mix_dh(dC1, a.f.M[0], B, T, J, b, t, q); break;                                    // h_fake
            case 1: s = mix_dM(dC1, a.f.h[0], B, T, J, b, t, q) + mix_dM(dC3, a.f.h[2], B, T, J, b, t, q); break;  // m_real
            case 2: s = mix_dh(dC3, a.f.M[2], B, T, J, b, t, q); break;                                    // h_real_p
            case 3: s = mix_dM(dC4, a.f.h[3], B, T, J, b, t, q); break;                                    // m_fake
            case 4: s = mix_dh(dC2, a.f.M[1], B, T, J, b, t, q) + mix_dh(dC4, a.f.M[3], B, T, J, b, t, q); break;  // h_fake_p
            default: s = mix_dM(dC2, a.f.h[1], B, T, J, b, t, q); break;                                   // m_real_p
        }
        out[y] = s * a.sc * gs;
    }
}

// four-problem counterparts of mixed_divergence_fwd / _bwd (sinkhorn.hip) for the history path
__global__ void mixed_sinkhorn_combine_fwd(const float* __restrict__ cost4, float* __restrict__ loss) {
    if (threadIdx.x == 0) loss[0] = ((cost4[0] + cost4[1]) - cost4[2]) - cost4[3];
}
__global__ void mixed_sinkhorn_combine_bwd(const float* __restrict__ gloss, float* __restrict__ gcost4) {
    if (threadIdx.x < 4) {
        const float g = gloss[0];
        gcost4[threadIdx.x] = threadIdx.x < 2 ? g : -g;
    }
}

static bool mix_shape_ok(int B, int64_t K, int T, int J) {
    return B > 0 && K > 0 && T >= 1 && J >= 1 && (int64_t)B * 2 <= (1 << 20);
}

struct MixWs {
    float* D3;            // [3,2B,2B]: D3 (forward) / g3 (backward)
    float* dC;            // [4,B,B]:   d loss / d Cmix of the history path
    float* gc;            // [4]:       gloss * w
    void* stage;
    size_t stage_bytes;
};

static MixWs mix_ws(void* ws, size_t ws_bytes, int B) {
    char* base = static_cast<char*>(ws);
    const size_t s3 = up256((size_t)12 * B * B * sizeof(float)), s4 = up256((size_t)4 * B * B * sizeof(float));
    MixWs w;
    w.D3 = reinterpret_cast<float*>(base);
    w.dC = reinterpret_cast<float*>(base + s3);
    w.gc = reinterpret_cast<float*>(base + s3 + s4);
    w.stage = base + s3 + s4 + 256;
    w.stage_bytes = ws_bytes - (s3 + s4 + 256);
    return w;
}

static MixFeats mix_feats(const float* h_fake, const float* m_real, const float* h_real_p, const float* m_fake,
                          const float* h_fake_p, const float* m_real_p) {
    return MixFeats{{h_fake, h_fake_p, h_real_p, h_fake_p}, {m_real, m_real_p, m_real, m_fake}};
}

}  // namespace kccot
using namespace kccot;

extern "C" size_t kccot_mixed_sinkhorn_loss_workspace_bytes(int B, int64_t K) {
    if (B <= 0 || K <= 0 || (int64_t)B * 2 > (1 << 20)) return 0;
    size_t stage = kccot_pairwise_cost3_workspace_bytes(2 * B, K);
    const size_t sk = kccot_sinkhorn_workspace_bytes(4, B), cb = kccot_pairwise_cost3_bwd_workspace_bytes(2 * B, K);
    if (sk > stage) stage = sk;
    if (cb > stage) stage = cb;
    return up256((size_t)12 * B * B * sizeof(float)) + up256((size_t)4 * B * B * sizeof(float)) + 256 + up256(stage);
}

extern "C" int kccot_mixed_sinkhorn_loss_fwd_f32(const float* R, const float* F, int B, int64_t K, float sc,
                                                 const float* h_fake, const float* m_real, const float* h_real_p,
                                                 const float* m_fake, const float* h_fake_p, const float* m_real_p,
                                                 int T, int J, float eps, int L, int Lmin, float thresh, unsigned flags,
                                                 float* Cmix, float* u_hist, float* v_hist, float* dCmix_unit,
                                                 float* cost4_out, int32_t* nits_out, float* loss_out, int32_t* ticket,
                                                 void* ws, size_t ws_bytes, kccot_stream_t stream) {
    // KCCOT_MIXED_CMIX_GIVEN: Cmix is an input (assembled by the caller, e.g. from the gathered row blocks of a
    // batch-sharded loss); R, F, K and the features are not read and the cost stage is skipped
    const bool given = (flags & KCCOT_MIXED_CMIX_GIVEN) != 0;
    if (given && flags != KCCOT_MIXED_CMIX_GIVEN)
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: CMIX_GIVEN takes no other flag (flags=%u)", flags);
    if (!given && (!R || !F || !h_fake || !m_real || !h_real_p || !m_fake || !h_fake_p || !m_real_p))
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: null input pointer");
    if (!Cmix || !cost4_out || !nits_out || !loss_out)
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: null output pointer");
    if (!(given ? (B > 0 && (int64_t)B * 2 <= (1 << 20)) : mix_shape_ok(B, K, T, J)) || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: bad arguments B=%d K=%lld T=%d J=%d L=%d eps=%g", B,
                    (long long)K, T, J, L, (double)eps);
    if ((u_hist == nullptr) != (v_hist == nullptr) || (dCmix_unit && u_hist))
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: give u_hist and v_hist together, or dCmix_unit, not both");
    if (dCmix_unit && !ticket) return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: the fused path needs the ticket");
    if (flags & (KCCOT_COST_GRAM_SUMS_ONLY | KCCOT_COST_FROM_GRAM_SUMS | KCCOT_COST_BICAUSAL_TERM_ONLY | KCCOT_COST_CAUSAL_ADD |
                 KCCOT_COST_RBF_SUM | KCCOT_COST_L1))
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_fwd: the Gram-sum split / term-only / causal-add / RBF_SUM / L1 flags do not apply");
    hipStream_t st = (hipStream_t)stream;
    void* stage = ws;
    size_t stage_bytes = ws_bytes;
    int rc;
    if (given) {
        // only the history path's solves use a workspace (kccot_sinkhorn_workspace_bytes(4, B): nothing grows with K)
        const size_t need = dCmix_unit ? 0 : kccot_sinkhorn_workspace_bytes(4, B);
        if (need && (!ws || ws_bytes < need))
            return fail(KCCOT_EWORKSPACE, "mixed_sinkhorn_loss_fwd: workspace %zu < %zu bytes (CMIX_GIVEN)", ws_bytes, need);
    } else {
        if (!ws || ws_bytes < kccot_mixed_sinkhorn_loss_workspace_bytes(B, K))
            return fail(KCCOT_EWORKSPACE, "mixed_sinkhorn_loss_fwd: workspace %zu < %zu bytes", ws_bytes,
                        kccot_mixed_sinkhorn_loss_workspace_bytes(B, K));
        const MixWs w = mix_ws(ws, ws_bytes, B);
        rc = kccot_pairwise_cost3_f32(R, F, 2 * B, K, sc, nullptr, nullptr, nullptr, nullptr, 1, 1, flags, w.D3, w.stage,
                                      w.stage_bytes, stream);
        if (rc) return rc;
        const int64_t n4 = 4 * (int64_t)B * B;
        hipLaunchKernelGGL(mixed_cost_finalize, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, st, (const float*)w.D3,
                           mix_feats(h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p), B, T, J, sc, Cmix);
        if ((rc = launch_status("mixed_cost_finalize"))) return rc;
        stage = w.stage;
        stage_bytes = w.stage_bytes;
    }
    if (dCmix_unit)
        return sinkhorn_fused_weighted(Cmix, 4, kMixW, B, eps, L, Lmin, thresh, cost4_out, nits_out, loss_out, ticket,
                                       dCmix_unit, st);
    rc = kccot_sinkhorn_fwd_f32(Cmix, 4, B, eps, L, Lmin, thresh, KCCOT_STOP_COUNT, u_hist, v_hist, cost4_out, nits_out,
                                nullptr, stage, stage_bytes, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(mixed_sinkhorn_combine_fwd, dim3(1), dim3(64), 0, st, (const float*)cost4_out, loss_out);
    return launch_status("mixed_sinkhorn_combine_fwd");
}

extern "C" int kccot_mixed_sinkhorn_loss_bwd_f32(const float* gloss, const float* R, const float* F, int B, int64_t K,
                                                 float sc, const float* h_fake, const float* m_real, const float* h_real_p,
                                                 const float* m_fake, const float* h_fake_p, const float* m_real_p,
                                                 int T, int J, float eps, int L, const float* Cmix, const float* u_hist,
                                                 const float* v_hist, const int32_t* nits, const float* dCmix_unit,
                                                 float* dF, float* dh_fake, float* dm_real, float* dh_real_p,
                                                 float* dm_fake, float* dh_fake_p, float* dm_real_p,
                                                 void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!gloss || !R || !F || !h_fake || !m_real || !h_real_p || !m_fake || !h_fake_p || !m_real_p)
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_bwd: null input pointer");
    if (!dCmix_unit && (!Cmix || !u_hist || !v_hist || !nits))
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_bwd: give dCmix_unit (fused forward) or Cmix, u_hist, v_hist, nits");
    if (!mix_shape_ok(B, K, T, J) || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "mixed_sinkhorn_loss_bwd: bad arguments B=%d K=%lld T=%d J=%d", B, (long long)K, T, J);
    if (!ws || ws_bytes < kccot_mixed_sinkhorn_loss_workspace_bytes(B, K))
        return fail(KCCOT_EWORKSPACE, "mixed_sinkhorn_loss_bwd: workspace %zu < %zu bytes", ws_bytes,
                    kccot_mixed_sinkhorn_loss_workspace_bytes(B, K));
    hipStream_t st = (hipStream_t)stream;
    const MixWs w = mix_ws(ws, ws_bytes, B);
    int rc;
    const float* dC = dCmix_unit;
    const float* gscale = gloss;
    if (!dCmix_unit) {
        // history path: gcost = gloss * {1,1,-1,-1} on the device, then the reverse sweep of the four problems
        hipLaunchKernelGGL(mixed_sinkhorn_combine_bwd, dim3(1), dim3(64), 0, st, gloss, w.gc);
        if ((rc = launch_status("mixed_sinkhorn_combine_bwd"))) return rc;
        rc = kccot_sinkhorn_bwd_f32(Cmix, u_hist, v_hist, nits, 4, B, eps, L, w.gc, w.dC, w.stage, w.stage_bytes, stream);
        if (rc) return rc;
        dC = w.dC;
        gscale = nullptr;
    }
    MixBwdArgs a{dC, gscale, mix_feats(h_fake, m_real, h_real_p, m_fake, h_fake_p, m_real_p), w.D3,
                 {dh_fake, dm_real, dh_real_p, dm_fake, dh_fake_p, dm_real_p}, B, T, J, sc};
    const int64_t total = 12 * (int64_t)B * B + 6 * (int64_t)B * T * J;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(mixed_cost_bwd, dim3((unsigned)blocks), dim3(256), 0, st, a);
    if ((rc = launch_status("mixed_cost_bwd"))) return rc;
    if (!dF) return 0;
    return kccot_pairwise_cost3_bwd_f32(w.D3, R, F, 2 * B, K, sc, nullptr, nullptr, nullptr, nullptr, 1, 1, dF, nullptr,
                                        nullptr, nullptr, nullptr, w.stage, w.stage_bytes, stream);
}
