// Sliced Wasserstein distance (squared, order 2) between two batches and its adjoint (include/kccot_swd.h; NOT reference
// behaviour).  The P x K direction matrix is never stored: every kernel that needs directions generates its tile in LDS from
// Philox4x32-10 + Box-Muller, once per workgroup, and contracts it on the f32-input MFMA (v_mfma_f32_32x32x2_f32: exact fp32
// products, one fixed accumulation chain per element).
//
//   swd_project      grid (chunks, npt, nrt), 4 waves.  A workgroup holds a K-chunk, PT = 64 projections and RT = 128 rows of
//                    [real; fake] (wave w: rows 32 w .. 32 w + 31).  Per step of KS = 64 columns: every lane loads its row's 8
//                    float4 (lane half h takes the columns 8 j + 4 h ..), the workgroup generates theta [64][64] into one of two
//                    LDS buffers (4 Philox groups per thread; sum theta^2 rides along in registers), one barrier, then 64 MFMA per
//                    wave with A = theta (M = projection) and B = the rows (N = row), so a store is 32 consecutive rows of one
//                    projection.  PT = 64 and not 128: at P = 128 two workgroups share a CU, and one's generation (VALU) runs
//                    under the other's MFMA; the rows are then read twice, the second time from L2.  Partials: part_x [chunk][P][2B], part_n [chunk][P].  Rows that do not fill a tile are zero
//                    columns of the same MFMA: there is no second code path.
//   swd_sort         one workgroup per projection: fp64 sum of the chunks in a fixed order (chunk groups in parallel, combined in
//                    order), times 1 / |theta| in fp64, rounded once; bitonic sort of (value, index) pairs of both planes in LDS,
//                    +inf padded; fp64 sum of the squared differences -> pp [p].
//   swd_finish       one workgroup: pp summed in a fixed order, / (P B).
//   swd_coef         coef [2B][Ppad] = +-(2 g / (P B)) (a_(r) - b_(r)) / |theta_p| at the samples of rank r, zero in the padding.
//   swd_backproject  grid (k tiles of KT = 128, row tiles), 4 waves (wave w: columns 32 w ..).  Per step of 64 projections theta
//                    [64][128] is generated into LDS, then d[row][k] += coef[row][p] theta[p][k] with A = coef (M = row), B = theta
//                    (N = k): one chain over p per element, stores are 32 consecutive k.
#include "common.h"
#include "../../include/kccot_swd.h"

namespace kccot {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int SWD_PT = 64, SWD_RT = 128, SWD_KS = 64, SWD_LDT = SWD_KS + 4;         // swd_project
constexpr int SWD_NPB = SWD_PT / 32, SWD_NGI = SWD_PT / 16;                          // its MFMA tiles per wave, Philox groups per thread
constexpr int SWD_KT = 128, SWD_PS = 64, SWD_LDB = SWD_KT + 4;                        // swd_backproject
constexpr int SWD_ST = 1024;                                                          // swd_sort: threads
constexpr int64_t SWD_KC = 512;
constexpr int SWD_MAX_CHUNKS = 1024;
constexpr int64_t SWD_MAX_K = (int64_t)1 << 40;

// ---- the generator ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void philox4x32_10(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ float swd_unit(uint32_t r) { return ((float)(r >> 9) + 0.5f) * 1.1920928955078125e-07f; }

__device__ __forceinline__ void swd_pair(uint32_t ra, uint32_t rb, float& z0, float& z1) {
    const float rad = sqrtf(-2.0f * logf(swd_unit(ra)));
    float s, c;
    sincospif(2.0f * swd_unit(rb), &s, &c);
    z0 = rad * c;
    z1 = rad * s;
}

// the elements 4 q .. 4 q + 3 of direction p
__device__ __forceinline__ float4 swd_group(uint32_t key0, uint32_t key1, int64_t q, uint32_t p) {
    uint32_t c0 = (uint32_t)((uint64_t)q & 0xffffffffu), c1 = (uint32_t)((uint64_t)q >> 32), c2 = p, c3 = 0;
    philox4x32_10(c0, c1, c2, c3, key0, key1);
    float4 z;
    swd_pair(c0, c1, z.x, z.y);
    swd_pair(c2, c3, z.z, z.w);
    return z;
}

__global__ __launch_bounds__(256) void swd_directions(uint32_t key0, uint32_t key1, int64_t K, int p_begin, float* __restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x, k = 4 * q;
    if (k >= K) return;
    const float4 z = swd_group(key0, key1, q, (uint32_t)(p_begin + (int)blockIdx.y));
    float* o = out + (int64_t)blockIdx.y * K + k;
    o[0] = z.x;
    if (k + 1 < K) o[1] = z.y;
    if (k + 2 < K) o[2] = z.z;
    if (k + 3 < K) o[3] = z.w;
}

// ---- forward: projections ------------------------------------------------------------------------------------------------------
template <bool ALIGNED>
__device__ __forceinline__ float4 swd_load4(const float* __restrict__ row, int64_t k, int64_t kend) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!row) return v;
    if (ALIGNED) {                                   // k, kend multiples of 4: the group is inside or outside as a whole
        if (k < kend) v = *reinterpret_cast<const float4*>(row + k);
    } else {
        if (k < kend) v.x = row[k];
        if (k + 1 < kend) v.y = row[k + 1];
        if (k + 2 < kend) v.z = row[k + 2];
        if (k + 3 < kend) v.w = row[k + 3];
    }
    return v;
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void swd_project(const float* __restrict__ real, const float* __restrict__ fake, int B, int64_t K,
                                                   int P, uint32_t key0, uint32_t key1, int64_t kc, float* __restrict__ part_x,
                                                   float* __restrict__ part_n) {
    __shared__ float th[2][SWD_PT * SWD_LDT];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, n = lane & 31, h = lane >> 5;
    const int chunk = blockIdx.x, p0 = blockIdx.y * SWD_PT, R = 2 * B;
    const int row = blockIdx.z * SWD_RT + w * 32 + n;
    const float* xrow = row < B ? real + (int64_t)row * K : (row < R ? fake + (int64_t)(row - B) * K : nullptr);
    const int64_t kbeg = (int64_t)chunk * kc, kend = (kbeg + kc < K) ? kbeg + kc : K;
    const int nsteps = (int)((kend - kbeg + SWD_KS - 1) / SWD_KS);
    const int gp = t >> 4, gq = t & 15;              // generation: projections gp + 16 i, Philox group gq of the step

    f32x16 acc[SWD_NPB];
#pragma unroll
    for (int i = 0; i < SWD_NPB; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;
    float n2[SWD_NGI];
#pragma unroll
    for (int i = 0; i < SWD_NGI; ++i) n2[i] = 0.f;

    for (int s = 0; s < nsteps; ++s) {
        const int64_t k0 = kbeg + (int64_t)s * SWD_KS;
        float4 xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) xv[j] = swd_load4<ALIGNED>(xrow, k0 + 8 * j + 4 * h, kend);
        float* buf = th[s & 1];
        const int64_t kg = k0 + 4 * gq;
#pragma unroll
        for (int i = 0; i < SWD_NGI; ++i) {
            float4 z = swd_group(key0, key1, kg >> 2, (uint32_t)(p0 + gp + 16 * i));
            if (kg >= kend) z.x = 0.f;
            if (kg + 1 >= kend) z.y = 0.f;
            if (kg + 2 >= kend) z.z = 0.f;
            if (kg + 3 >= kend) z.w = 0.f;
            n2[i] = fmaf(z.w, z.w, fmaf(z.z, z.z, fmaf(z.y, z.y, fmaf(z.x, z.x, n2[i]))));
            *reinterpret_cast<float4*>(buf + (gp + 16 * i) * SWD_LDT + 4 * gq) = z;
        }
        __syncthreads();                             // the one barrier of a step: the other buffer was read a step ago
#pragma unroll
        for (int j = 0; j < 8; ++j) {
#pragma unroll
            for (int pb = 0; pb < SWD_NPB; ++pb) {
                const float4 a = *reinterpret_cast<const float4*>(buf + (pb * 32 + n) * SWD_LDT + 8 * j + 4 * h);
                acc[pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, xv[j].x, acc[pb], 0, 0, 0);
                acc[pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, xv[j].y, acc[pb], 0, 0, 0);
                acc[pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, xv[j].z, acc[pb], 0, 0, 0);
                acc[pb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, xv[j].w, acc[pb], 0, 0, 0);
            }
        }
    }
    // lane (n, h), register v of tile pb: projection p0 + 32 pb + 8 (v / 4) + 4 h + v % 4, row `row`
    if (row < R) {
#pragma unroll
        for (int pb = 0; pb < SWD_NPB; ++pb)
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int p = p0 + pb * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
                if (p < P) part_x[((int64_t)chunk * P + p) * R + row] = acc[pb][v];
            }
    }
    if (blockIdx.z == 0) {
#pragma unroll
        for (int i = 0; i < SWD_NGI; ++i) {
            const float s2 = seg_sum<16>(n2[i]);
            const int p = p0 + gp + 16 * i;
            if (gq == 0 && p < P) part_n[(int64_t)chunk * P + p] = s2;
        }
    }
}

// ---- forward: chunk sum, sort, squared differences -------------------------------------------------------------------------
__global__ __launch_bounds__(SWD_ST) void swd_sort(const float* __restrict__ part_x, const float* __restrict__ part_n, int chunks,
                                                   int B, int P, int NP, float* __restrict__ proj_out, int32_t* __restrict__ order_out,
                                                   float* __restrict__ inv_norm_out, double* __restrict__ pp) {
    __shared__ double dsum[2 * KCCOT_SWD_MAX_B + 1];
    __shared__ double dgrp[SWD_ST];
    __shared__ float key[2][KCCOT_SWD_MAX_B];
    __shared__ int idx[2][KCCOT_SWD_MAX_B];
    __shared__ double dw[SWD_ST / 64];
    const int t = threadIdx.x, p = blockIdx.x, R = 2 * B, RT = R + 1;     // "row" R is the squared norm
    // G groups of RP threads: group g adds the chunks g, g + G, .. of its row in order, then the G sums are added in order
    int RP = 1;
    while (RP < RT && RP < SWD_ST) RP <<= 1;
    const int G = SWD_ST / RP, g = t / RP;
    for (int r = t % RP; r < RT; r += RP) {
        const float* src = r < R ? part_x + (int64_t)p * R + r : part_n + p;
        const int64_t stride = r < R ? (int64_t)P * R : (int64_t)P;
        double s = 0.0;
        int c = g;
        for (; c + 7 * G < chunks; c += 8 * G) {                          // eight loads in flight, added in order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = src[(int64_t)(c + u * G) * stride];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += (double)v[u];
        }
        for (; c < chunks; c += G) s += (double)src[(int64_t)c * stride];
        if (G == 1) dsum[r] = s;
        else dgrp[t] = s;
    }
    __syncthreads();
    if (G > 1 && t < RT) {
        double s = 0.0;
        for (int q = 0; q < G; ++q) s += dgrp[q * RP + t];
        dsum[t] = s;
    }
    __syncthreads();
    const double inv = 1.0 / sqrt(dsum[R]);
    if (t == 0) inv_norm_out[p] = (float)inv;
    for (int e = t; e < 2 * NP; e += SWD_ST) {
        const int s = e >= NP, i = e - s * NP;
        float v = __builtin_inff();
        if (i < B) {
            v = (float)(dsum[s * B + i] * inv);
            proj_out[((int64_t)s * P + p) * B + i] = v;
        }
        key[s][i] = v;
        idx[s][i] = i;
    }
    __syncthreads();
    for (int k = 2; k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int e = t; e < NP; e += SWD_ST) {           // NP / 2 pairs in each plane
                const int s = e >= (NP >> 1), q = e - s * (NP >> 1);
                const int i = ((q & ~(j - 1)) << 1) | (q & (j - 1)), l = i | j;
                const float ki = key[s][i], kl = key[s][l];
                const int ii = idx[s][i], il = idx[s][l];
                const bool gt = ki > kl || (ki == kl && ii > il);
                if (gt == ((i & k) == 0)) {
                    key[s][i] = kl, key[s][l] = ki;
                    idx[s][i] = il, idx[s][l] = ii;
                }
            }
            __syncthreads();
        }
    double ss = 0.0;
    for (int r = t; r < B; r += SWD_ST) {
        const float d = key[0][r] - key[1][r];
        ss += (double)d * (double)d;
        order_out[(int64_t)p * B + r] = idx[0][r];
        order_out[((int64_t)P + p) * B + r] = idx[1][r];
    }
    ss = wave_sum_d(ss);
    if ((t & 63) == 0) dw[t >> 6] = ss;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int w = 0; w < SWD_ST / 64; ++w) tot += dw[w];
        pp[p] = tot;
    }
}

__global__ __launch_bounds__(256) void swd_finish(const double* __restrict__ pp, int P, int B, float* __restrict__ swd_out) {
    __shared__ double dw[4];
    const int t = threadIdx.x;
    double s = 0.0;
    for (int p = t; p < P; p += 256) s += pp[p];
    s = wave_sum_d(s);
    if ((t & 63) == 0) dw[t >> 6] = s;
    __syncthreads();
    if (t == 0) swd_out[0] = (float)(((dw[0] + dw[1]) + (dw[2] + dw[3])) / ((double)P * (double)B));
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swd_coef(const float* __restrict__ gswd, const float* __restrict__ proj,
                                                const int32_t* __restrict__ order, const float* __restrict__ inv_norm, int B, int P,
                                                int Ppad, float* __restrict__ coef) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)B * Ppad) return;
    const int p = (int)(e % Ppad), r = (int)(e / Ppad);
    if (p >= P) {
        coef[(int64_t)r * Ppad + p] = 0.f;
        coef[(int64_t)(B + r) * Ppad + p] = 0.f;
        return;
    }
    const int i = order[(int64_t)p * B + r], j = order[((int64_t)P + p) * B + r];
    const float d = proj[(int64_t)p * B + i] - proj[((int64_t)P + p) * B + j];
    const float sc = (float)(2.0 * (double)gswd[0] / ((double)P * (double)B));
    const float v = sc * d * inv_norm[p];
    coef[(int64_t)i * Ppad + p] = v;
    coef[(int64_t)(B + j) * Ppad + p] = -v;
}

// rows [row_begin, row_end) of [real; fake]; a workgroup holds nrb <= 4 blocks of 32 of them
__global__ __launch_bounds__(256) void swd_backproject(const float* __restrict__ coef, int Ppad, int row_begin, int row_end, int B,
                                                       int64_t K, uint32_t key0, uint32_t key1, float* __restrict__ dreal,
                                                       float* __restrict__ dfake) {
    __shared__ float th[2][SWD_PS * SWD_LDB];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, n = lane & 31, h = lane >> 5;
    const int64_t kt0 = (int64_t)blockIdx.x * SWD_KT;
    const int rbase = row_begin + blockIdx.y * 128;
    const int left = row_end - rbase, nrb = left >= 128 ? 4 : (left + 31) / 32;
    const int gk = t & 31, gpl = t >> 5;             // generation: Philox group gk of the tile, projections gpl + 8 i
    const float* crow[4];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
        const int row = rbase + rb * 32 + n;
        crow[rb] = row < row_end ? coef + (int64_t)row * Ppad + 4 * h : nullptr;
    }
    f32x16 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[i][v] = 0.f;

    const int nsteps = Ppad / SWD_PS;
    for (int s = 0; s < nsteps; ++s) {
        const int ps = s * SWD_PS;
        float* buf = th[s & 1];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float4 z = swd_group(key0, key1, (kt0 >> 2) + gk, (uint32_t)(ps + gpl + 8 * i));
            *reinterpret_cast<float4*>(buf + (gpl + 8 * i) * SWD_LDB + 4 * gk) = z;
        }
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < 8; ++j) {
            float4 cf[4];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
                cf[rb] = (rb < nrb && crow[rb]) ? *reinterpret_cast<const float4*>(crow[rb] + ps + 8 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float* bp = buf + (8 * j + 4 * h) * SWD_LDB + w * 32 + n;
            const float b0 = bp[0], b1 = bp[SWD_LDB], b2 = bp[2 * SWD_LDB], b3 = bp[3 * SWD_LDB];
#pragma unroll
            for (int rb = 0; rb < 4; ++rb)
                if (rb < nrb) {
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[rb].x, b0, acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[rb].y, b1, acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[rb].z, b2, acc[rb], 0, 0, 0);
                    acc[rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(cf[rb].w, b3, acc[rb], 0, 0, 0);
                }
        }
    }
    // lane (n, h), register v of block rb: row rbase + 32 rb + 8 (v / 4) + 4 h + v % 4, column kt0 + 32 w + n
    const int64_t k = kt0 + w * 32 + n;
    if (k >= K) return;
#pragma unroll
    for (int rb = 0; rb < 4; ++rb)
        if (rb < nrb) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = rbase + rb * 32 + 8 * (v >> 2) + 4 * h + (v & 3);
                if (row < row_end) {
                    if (row < B) dreal[(int64_t)row * K + k] = acc[rb][v];
                    else dfake[(int64_t)(row - B) * K + k] = acc[rb][v];
                }
            }
        }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct SwdPlan {
    int64_t kc;
    int chunks, npt, nrt, np, ppad;
    size_t off_n, off_pp, fwd_bytes, bwd_bytes;
};

int swd_shape(const char* who, int B, int64_t K, int P) {
    if (B < 1 || K < 1 || P < 1) return fail(KCCOT_EINVAL, "%s: bad shape B=%d K=%lld P=%d", who, B, (long long)K, P);
    if (B > KCCOT_SWD_MAX_B) return fail(KCCOT_EUNSUPPORTED, "%s: B=%d > %d", who, B, KCCOT_SWD_MAX_B);
    if (P > KCCOT_SWD_MAX_P) return fail(KCCOT_EUNSUPPORTED, "%s: P=%d > %d", who, P, KCCOT_SWD_MAX_P);
    if (K > SWD_MAX_K) return fail(KCCOT_EUNSUPPORTED, "%s: K=%lld > 2^40", who, (long long)K);
    return 0;
}

SwdPlan swd_plan(int B, int64_t K, int P) {
    SwdPlan pl;
    pl.kc = SWD_KC;
    while ((K + pl.kc - 1) / pl.kc > SWD_MAX_CHUNKS) pl.kc *= 2;
    pl.chunks = (int)((K + pl.kc - 1) / pl.kc);
    pl.npt = (P + SWD_PT - 1) / SWD_PT;
    pl.nrt = (2 * B + SWD_RT - 1) / SWD_RT;
    pl.np = 1;
    while (pl.np < B) pl.np <<= 1;
    pl.ppad = (P + SWD_PS - 1) / SWD_PS * SWD_PS;
    pl.off_n = up256((size_t)pl.chunks * P * 2 * B * sizeof(float));
    pl.off_pp = pl.off_n + up256((size_t)pl.chunks * P * sizeof(float));
    pl.fwd_bytes = pl.off_pp + up256((size_t)P * sizeof(double));
    pl.bwd_bytes = up256((size_t)2 * B * pl.ppad * sizeof(float));
    return pl;
}

bool swd_overlap(const void* p, size_t pb, const void* q, size_t qb) {
    if (!p || !q) return false;
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return a < b + qb && b < a + pb;
}

}  // namespace
}  // namespace kccot

using namespace kccot;

extern "C" size_t kccot_swd_workspace_bytes(int B, int64_t K, int P) {
    if (B < 1 || K < 1 || P < 1 || B > KCCOT_SWD_MAX_B || P > KCCOT_SWD_MAX_P || K > SWD_MAX_K) return 0;
    const SwdPlan pl = swd_plan(B, K, P);
    return pl.fwd_bytes > pl.bwd_bytes ? pl.fwd_bytes : pl.bwd_bytes;
}

extern "C" int kccot_swd_plan(int B, int64_t K, int P, int* out) {
    const char* who = "kccot_swd_plan";
    if (!out) return fail(KCCOT_EINVAL, "%s: null out", who);
    if (int rc = swd_shape(who, B, K, P)) return rc;
    const SwdPlan pl = swd_plan(B, K, P);
    out[0] = (int)pl.kc, out[1] = pl.chunks, out[2] = SWD_PT, out[3] = SWD_RT, out[4] = pl.npt, out[5] = pl.nrt, out[6] = pl.np;
    out[7] = SWD_KT;
    return 0;
}

extern "C" int kccot_swd_directions_f32(uint64_t seed, int64_t K, int p_begin, int p_count, float* out, kccot_stream_t stream) {
    const char* who = "kccot_swd_directions_f32";
    if (!out) return fail(KCCOT_EINVAL, "%s: null output pointer", who);
    if (K < 1 || p_count < 1 || p_begin < 0)
        return fail(KCCOT_EINVAL, "%s: bad shape K=%lld p_begin=%d p_count=%d", who, (long long)K, p_begin, p_count);
    if (p_count > KCCOT_SWD_MAX_P || p_begin > KCCOT_SWD_MAX_P - p_count)
        return fail(KCCOT_EUNSUPPORTED, "%s: p_begin + p_count = %lld > %d", who, (long long)p_begin + p_count, KCCOT_SWD_MAX_P);
    if (K > SWD_MAX_K) return fail(KCCOT_EUNSUPPORTED, "%s: K=%lld > 2^40", who, (long long)K);
    const dim3 grid((unsigned)((K + 1023) / 1024), (unsigned)p_count);
    hipLaunchKernelGGL(swd_directions, grid, dim3(256), 0, (hipStream_t)stream, (uint32_t)(seed & 0xffffffffu),
                       (uint32_t)(seed >> 32), K, p_begin, out);
    return launch_status(who);
}

extern "C" int kccot_swd_fwd_f32(const float* real, const float* fake, int B, int64_t K, int P, uint64_t seed, float* proj_out,
                                 int32_t* order_out, float* inv_norm_out, float* swd_out, void* ws, size_t ws_bytes,
                                 kccot_stream_t stream) {
    const char* who = "kccot_swd_fwd_f32";
    if (!real || !fake) return fail(KCCOT_EINVAL, "%s: null input pointer", who);
    if (!proj_out || !order_out || !inv_norm_out || !swd_out) return fail(KCCOT_EINVAL, "%s: null output pointer", who);
    if (int rc = swd_shape(who, B, K, P)) return rc;
    const size_t vb = (size_t)B * (size_t)K * 4, pb = (size_t)2 * P * B * 4, nb = (size_t)P * 4;
    const void* outs[4] = {proj_out, order_out, inv_norm_out, swd_out};
    const size_t ob[4] = {pb, pb, nb, 4};
    for (int a = 0; a < 4; ++a) {
        if (swd_overlap(outs[a], ob[a], real, vb) || swd_overlap(outs[a], ob[a], fake, vb))
            return fail(KCCOT_EINVAL, "%s: an output must not alias an input", who);
        for (int b = a + 1; b < 4; ++b)
            if (swd_overlap(outs[a], ob[a], outs[b], ob[b])) return fail(KCCOT_EINVAL, "%s: two outputs alias each other", who);
    }
    const SwdPlan pl = swd_plan(B, K, P);
    const size_t need = kccot_swd_workspace_bytes(B, K, P);
    if (!ws || ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", who, ws_bytes, need);
    if ((uintptr_t)ws & 15) return fail(KCCOT_EINVAL, "%s: the workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    float* part_x = (float*)ws;
    float* part_n = (float*)((char*)ws + pl.off_n);
    double* pp = (double*)((char*)ws + pl.off_pp);
    const uint32_t key0 = (uint32_t)(seed & 0xffffffffu), key1 = (uint32_t)(seed >> 32);
    const bool aligned = K % 4 == 0 && ((uintptr_t)real & 15) == 0 && ((uintptr_t)fake & 15) == 0;
    const dim3 grid((unsigned)pl.chunks, (unsigned)pl.npt, (unsigned)pl.nrt);
    if (aligned)
        hipLaunchKernelGGL(swd_project<true>, grid, dim3(256), 0, st, real, fake, B, K, P, key0, key1, pl.kc, part_x, part_n);
    else
        hipLaunchKernelGGL(swd_project<false>, grid, dim3(256), 0, st, real, fake, B, K, P, key0, key1, pl.kc, part_x, part_n);
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(swd_sort, dim3((unsigned)P), dim3(SWD_ST), 0, st, (const float*)part_x, (const float*)part_n, pl.chunks, B, P,
                       pl.np, proj_out, order_out, inv_norm_out, pp);
    if (int rc = launch_status(who)) return rc;
    hipLaunchKernelGGL(swd_finish, dim3(1), dim3(256), 0, st, (const double*)pp, P, B, swd_out);
    return launch_status(who);
}

extern "C" int kccot_swd_bwd_f32(const float* gswd, const float* proj, const int32_t* order, const float* inv_norm, int B,
                                 int64_t K, int P, uint64_t seed, float* dreal, float* dfake, void* ws, size_t ws_bytes,
                                 kccot_stream_t stream) {
    const char* who = "kccot_swd_bwd_f32";
    if (!gswd || !proj || !order || !inv_norm) return fail(KCCOT_EINVAL, "%s: null input pointer", who);
    if (!dreal && !dfake) return fail(KCCOT_EINVAL, "%s: null output pointers (give dreal, dfake or both)", who);
    if (int rc = swd_shape(who, B, K, P)) return rc;
    const size_t vb = (size_t)B * (size_t)K * 4, pb = (size_t)2 * P * B * 4, nb = (size_t)P * 4;
    const void* ins[4] = {gswd, proj, order, inv_norm};
    const size_t ib[4] = {4, pb, pb, nb};
    for (int a = 0; a < 4; ++a)
        if (swd_overlap(dreal, vb, ins[a], ib[a]) || swd_overlap(dfake, vb, ins[a], ib[a]))
            return fail(KCCOT_EINVAL, "%s: an output must not alias an input", who);
    if (swd_overlap(dreal, vb, dfake, vb)) return fail(KCCOT_EINVAL, "%s: dreal and dfake alias each other", who);
    const SwdPlan pl = swd_plan(B, K, P);
    if ((K + SWD_KT - 1) / SWD_KT > 2147483647LL) return fail(KCCOT_EUNSUPPORTED, "%s: K=%lld too large", who, (long long)K);
    const size_t need = kccot_swd_workspace_bytes(B, K, P);
    if (!ws || ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", who, ws_bytes, need);
    if ((uintptr_t)ws & 15) return fail(KCCOT_EINVAL, "%s: the workspace must be 16-byte aligned", who);
    hipStream_t st = (hipStream_t)stream;
    float* coef = (float*)ws;
    const int64_t ne = (int64_t)B * pl.ppad;
    hipLaunchKernelGGL(swd_coef, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, gswd, proj, order, inv_norm, B, P, pl.ppad,
                       coef);
    if (int rc = launch_status(who)) return rc;
    const int row_begin = dreal ? 0 : B, row_end = dfake ? 2 * B : B;
    const dim3 grid((unsigned)((K + SWD_KT - 1) / SWD_KT), (unsigned)((row_end - row_begin + 127) / 128));
    hipLaunchKernelGGL(swd_backproject, grid, dim3(256), 0, st, (const float*)coef, pl.ppad, row_begin, row_end, B, K,
                       (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), dreal, dfake);
    return launch_status(who);
}
