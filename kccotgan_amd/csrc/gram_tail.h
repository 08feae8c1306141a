// The tail of the Gram paths of the cost assembly (cost_mfma.hip, cost_tiled.hip, cost_tile256.hip, cost_rows.hip), once:
// the fp64 sum over the K-chunks of the partial tiles, the loss's distances from ten Gram entries, and -- for the two
// paths that tile the stack [real ; fake - real] by pairs of panels -- the plan's sizes, the reduce and finalize kernels and
// the host driver with its split at the fp64 sums.  What differs between those two (the rows of a panel, where the Gram
// entry of two stack rows sits, which sums are never computed) is a layout struct next to each path's partial kernels.
#pragma once
#include "common.h"
#include "cost_internal.h"

namespace kccot {

// fp64 sum over the chunks, fixed order; eight loads in flight.  p: entry e of the first chunk; stride: elements from one
// chunk to the next; nchunk: the non-empty chunks
__device__ __forceinline__ double gram_chunk_sum(const float* __restrict__ p, int stride, int nchunk) {
    double s = 0.0;
    int c = 0;
    for (; c + 8 <= nchunk; c += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = p[(int64_t)(c + i) * stride];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += (double)v[i];
    }
    for (; c < nchunk; ++c) s += (double)p[(int64_t)c * stride];
    return s;
}

// Squared distance of problem p (0: xy, 1: xx, 2: yy; gan_utils.py:221-223) between samples i and j from the Gram entries of
// the stack [X ; E], E = Y - X (the pair-difference form): g = x.x, e = e.e, x_ab = x_a.e_b; diag: i and j are the same sample.
// With y = x + e:  |x_i - y_j|^2 = |x_i - x_j|^2 + e_jj - 2 (x_ij - x_jj),  |y_i - y_j|^2 = |x_i - x_j|^2 + |e_i - e_j|^2 + 2 (x_i - x_j).(e_i - e_j)
// -- the near-regime diagonal of C_xy is e_jj itself, not a difference of large norms.
// gram_loss_distance is what a finalize calls: the distance clamped at 0.  gram_finalize_body (cost_mfma.hip) calls the two
// halves itself, because its clamp also serves its GRAM_XY and GRAM_SAME branches: through the clamped form (a second clamp
// behind the branches, or one clamp per branch) gram_finalize came out 8 or 33 instructions longer.
// The ten entries come by value.  The epilogue the tiled finalizes repeat (scale, causal_tile16, store) is NOT here: as a
// function of this header, by value too, it cost each of them 3 to 7 more spilled SGPRs (profiles/gram_tail_refactor_isa.json).
__device__ __forceinline__ double gram_loss_distance_raw(int p, bool diag, double g_ii, double g_jj, double g_ij, double e_ii,
                                                         double e_jj, double e_ij, double x_ii, double x_jj, double x_ij,
                                                         double x_ji) {
    const double dxx = diag ? 0.0 : g_ii + g_jj - 2.0 * g_ij;
    const double dxy = dxx + e_jj - 2.0 * (x_ij - x_jj);
    const double dee = e_ii + e_jj - 2.0 * e_ij;
    const double dyy = diag ? 0.0 : dxx + dee + 2.0 * (x_ii - x_ij - x_ji + x_jj);
    return (p == 1) ? dxx : (p == 0 ? dxy : dyy);
}
// a squared distance; rounding of the Gram terms may leave -tiny
__device__ __forceinline__ double gram_clamp0(double D) { return D < 0.0 ? 0.0 : D; }
__device__ __forceinline__ double gram_loss_distance(int p, bool diag, double g_ii, double g_jj, double g_ij, double e_ii,
                                                     double e_jj, double e_ij, double x_ii, double x_jj, double x_ij,
                                                     double x_ji) {
    return gram_clamp0(gram_loss_distance_raw(p, diag, g_ii, g_jj, g_ij, e_ii, e_jj, e_ij, x_ii, x_jj, x_ij, x_ji));
}

// ---- the stack [real ; fake - real] in pairs (pa <= pb) of panels: cost_tiled.hip (128 rows), cost_tile256.hip (256 rows) ----
// A layout struct L gives: ELEMS (entries of a pair's tile), gram(gs, nt, a, b) (the Gram entry of stack rows a, b) and
// never_computed(nt, q, e) (entry e of pair q is written by no partial kernel: its sum is defined as 0).
struct StackPlan { int nx, nt, npairs, nchunk; int64_t chunk; size_t part_bytes, gsum_bytes, extra_bytes, ws_bytes; };

// grid (ELEMS / 256, pairs).  nstride: chunk slots per pair; nchunk: the non-empty ones
template <class L>
__global__ __launch_bounds__(256) void gram_stack_reduce(const float* __restrict__ part, int nstride, int nchunk,
                                                         double* __restrict__ gsum, int nt) {
    const int q = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (L::never_computed(nt, q, e)) { gsum[(int64_t)q * L::ELEMS + e] = 0.0; return; }
    gsum[(int64_t)q * L::ELEMS + e] = gram_chunk_sum(part + (int64_t)q * nstride * L::ELEMS + e, L::ELEMS, nchunk);
}

struct StackFin {
    const double* gsum;
    int B, nt;
    float* out[3];
    const float* h[3];
    const float* M[3];
    float sc;
    int T, J;
};

// One 16 x 16 output tile per block; blockIdx.z = problem (xy, xx, yy)
template <class L>
__global__ __launch_bounds__(256) void gram_stack_finalize(StackFin f) {
    __shared__ __attribute__((aligned(16))) float sh[CAUSAL_TILE * CAUSAL_PITCH];
    __shared__ __attribute__((aligned(16))) float sm[CAUSAL_TILE * CAUSAL_PITCH];
    const int p = blockIdx.z, B = f.B, nt = f.nt;
    const int i0 = blockIdx.y * CAUSAL_TILE, j0 = blockIdx.x * CAUSAL_TILE;
    const int i = i0 + (threadIdx.x >> 4), j = j0 + (threadIdx.x & 15);      // B % 16 == 0: always in range
    const double* G = f.gsum;
    const double g_ii = L::gram(G, nt, i, i), g_jj = L::gram(G, nt, j, j), g_ij = L::gram(G, nt, i, j);
    const double e_ii = L::gram(G, nt, B + i, B + i), e_jj = L::gram(G, nt, B + j, B + j), e_ij = L::gram(G, nt, B + i, B + j);
    const double x_ii = L::gram(G, nt, i, B + i), x_jj = L::gram(G, nt, j, B + j);
    const double x_ij = L::gram(G, nt, i, B + j), x_ji = L::gram(G, nt, j, B + i);
    const double D = gram_loss_distance(p, i == j, g_ii, g_jj, g_ij, e_ii, e_jj, e_ij, x_ii, x_jj, x_ij, x_ji);
    float c = (float)D * f.sc;
    if (f.h[p]) c += causal_tile16(f.h[p], f.M[p], i0, j0, B, B, f.T, f.J, sh, sm) * f.sc;
    f.out[p][(int64_t)i * B + j] = c;
}

// The host half the two paths share: workspace [part | gsum | extra], stage 0: everything; 1: stop after the fp64 sums; 2:
// finalize only.  partials(part, extra) launches the path's partial-tile kernels and returns their launch status.
template <class L, class Partials>
int run_gram_stack(const char* who, const StackPlan& pl, const CostBatch& cb, int64_t K, float sc, int T, int J, void* ws,
                   size_t ws_bytes, hipStream_t st, int stage, Partials partials) {
    const int B = cb.p[0].Bx;
    if (!ws || ws_bytes < pl.ws_bytes)
        return fail(KCCOT_EWORKSPACE, "pairwise_cost3(%s): workspace %zu < required %zu", who, ws_bytes, pl.ws_bytes);
    float* part = static_cast<float*>(ws);
    double* gsum = reinterpret_cast<double*>(static_cast<char*>(ws) + pl.part_bytes);
    float* extra = reinterpret_cast<float*>(static_cast<char*>(ws) + pl.part_bytes + pl.gsum_bytes);
    int rc;
    if (stage != 2) {
        if ((rc = partials(part, extra))) return rc;
        const int nvalid = (int)((K + pl.chunk - 1) / pl.chunk);
        hipLaunchKernelGGL(gram_stack_reduce<L>, dim3(L::ELEMS / 256, pl.npairs), dim3(256), 0, st, (const float*)part, pl.nchunk,
                           nvalid, gsum, pl.nt);
        if ((rc = launch_status("gram_stack_reduce"))) return rc;
        if (stage == 1) return 0;
    }
    StackFin f{};
    f.gsum = gsum; f.B = B; f.nt = pl.nt; f.sc = sc; f.T = T; f.J = J;
    for (int p = 0; p < 3; ++p) { f.out[p] = cb.p[p].out; f.h[p] = cb.p[p].h1; f.M[p] = cb.p[p].M1; }
    hipLaunchKernelGGL(gram_stack_finalize<L>, dim3(B / CAUSAL_TILE, B / CAUSAL_TILE, 3), dim3(256), 0, st, f);
    return launch_status("gram_stack_finalize");
}

}  // namespace kccot
