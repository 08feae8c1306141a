// What the two tile walks -- dsigma_tile (smooth_sigma.hip) and aniso_tile (smooth_aniso.hip) -- share.  A workgroup of TILE_NT
// threads owns, of one sample, a tile of tt rows of T, wt columns of W and ct channels and a segment of hs image rows, and walks
// along H.  ONE copy of: the tiling rule (tile_plan: the search and its cost model), the geometry a plan
// hands a kernel (TileGeom), the largest-grid search behind the workspace sizes, REFLECT, and the kernel that adds the
// per-workgroup fp64 partials in a fixed order (tile_combine).
// The kernels stay apart (a compile-time T radius and two fields there; a run-time one, LDS tap tables and three fields here),
// and so do the pieces of their bodies that read alike: the decode of blockIdx.x, the owned positions, u, the element walk of
// the T stage and the store of the partials.  Each was tried as a force-inlined function of this header; each, on its own,
// changed the emitted code of most instantiations and the spill counts of some.
#pragma once
#include "common.h"
#include <stdint.h>

namespace kccot {

constexpr int TILE_NT = 256;    // threads of a tile-walk workgroup

// ---- the tiling ----------------------------------------------------------------------------------------------------------------
// What a caller's search differs in.
struct TileSearch {
    int B, H, T, W, C;          // the extents in the kernel's view of the call
    int tb, ta, rw, rh;         // halo: rows of T before / after the piece, columns of W each side, planes of H each side
    int64_t max_items;          // owned positions of a workgroup at most (NI x TILE_NT)
    int nfields;                // tt x pitch fields in LDS behind the T stage
    size_t lds_max;             // dynamic LDS a tiling may take
    bool ni_pow2;               // NI = items / TILE_NT rounded up (false), or from there to the next power of two (true)
};

struct TilePlan { int tt, wt, ct, hs, ni; size_t lds; int64_t grid; bool ok; };

inline TilePlan tile_plan(const TileSearch& s) {
    TilePlan best{};
    double best_cost = 1e300;
    // halving cuts of every extent; the first (largest) tile of equal cost wins
    for (int ct = s.C;; ct = (ct + 1) / 2) {
        for (int wt = s.W;; wt = (wt + 1) / 2) {
            for (int tt = s.T;; tt = (tt + 1) / 2) {
                const int64_t items = (int64_t)tt * wt * ct;
                const int64_t pitch = (int64_t)(wt + 2 * s.rw) * ct;
                const int64_t lds = (2 * (int64_t)(tt + s.tb + s.ta) * pitch + s.nfields * (int64_t)tt * pitch) * 4;
                if (items <= s.max_items && lds <= (int64_t)s.lds_max) {
                    int ni = (int)((items + TILE_NT - 1) / TILE_NT);
                    if (s.ni_pow2)
                        for (ni = 1; (int64_t)ni * TILE_NT < items;) ni *= 2;
                    const int64_t ntile = (int64_t)((s.T + tt - 1) / tt) * ((s.W + wt - 1) / wt) * ((s.C + ct - 1) / ct);
                    for (int hs = s.H;; hs = (hs + 1) / 2) {
                        const int nseg = (s.H + hs - 1) / hs;
                        const int64_t grid = (int64_t)s.B * nseg * ntile;
                        // reads per owned element: the three halos; the ragged last tiles and the idle lanes of a tile that
                        // does not fill its NI x 256 positions; a channel cut leaves ct of every C consecutive floats useful
                        const double ragged = (double)ntile * (double)items * nseg * hs / ((double)s.T * s.W * s.C * s.H);
                        const double idle = (double)(ni * TILE_NT) / (double)items;
                        const double strided = (double)(s.C < 16 ? s.C : 16) / (double)(ct < 16 ? ct : 16);
                        const double over = (1.0 + (double)(s.tb + s.ta) / tt) * (1.0 + 2.0 * s.rw / wt) * (1.0 + 2.0 * s.rh / hs) *
                                            ragged * idle * strided;
                        // workgroups per CU (256 CUs) the chip should see: two where a shorter segment costs halo planes, eight
                        // where it costs nothing (no H window); the measurements are in DESIGN.md section 4.5.3
                        const double fill = (double)grid / (s.rh ? 512.0 : 2048.0);
                        const double cost = over * (fill >= 1.0 ? 1.0 : 1.0 / fill);
                        if (cost < best_cost && grid <= 0x7fffffff) {
                            best_cost = cost;
                            best = TilePlan{tt, wt, ct, hs, ni, (size_t)lds, grid, true};
                        }
                        if (hs == 1) break;
                    }
                }
                if (tt == 1) break;
            }
            if (wt == 1) break;
        }
        if (ct == 1) break;
    }
    return best;
}

// the tile geometry of a plan in the kernel's view of the shape: what a launch hands its kernel and what a plan query reports
struct TileGeom {
    int H, T, W, C;
    int tt, wt, ct, hs;         // tile extents along T, W, C and the segment along H
    int ntt, ntw, ntc, nseg;
};

inline TileGeom tile_geometry(const TileSearch& s, const TilePlan& pl) {
    return TileGeom{s.H, s.T, s.W, s.C, pl.tt, pl.wt, pl.ct, pl.hs, (s.T + pl.tt - 1) / pl.tt, (s.W + pl.wt - 1) / pl.wt,
                    (s.C + pl.ct - 1) / pl.ct, (s.H + pl.hs - 1) / pl.hs};
}

// The largest grid any plan launches at a shape (a workspace holds partials for it).  `plans(visit)` calls visit(plan) for every
// plan the caller can launch there: up to a million steps of the search, so each call site keeps the last shape's answer
// (`last`: one entry, thread_local at the call site).
struct TileGridCache { int key[5]; int64_t g; };

template <class Plans>
int64_t tile_largest_grid(TileGridCache& last, int B, int H, int T, int W, int C, Plans plans) {
    if (last.key[0] == B && last.key[1] == H && last.key[2] == T && last.key[3] == W && last.key[4] == C) return last.g;
    int64_t g = 1;
    plans([&g](const TilePlan& p) { if (p.ok && p.grid > g) g = p.grid; });
    last = {{B, H, T, W, C}, g};
    return g;
}

// ---- in the kernels ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int tile_reflect(int p, int len) {
    p = p < 0 ? -p : (p >= len ? 2 * (len - 1) - p : p);
    return p < 0 ? 0 : (p > len - 1 ? len - 1 : p);     // (positions only a masked output of a ragged tile asks for)
}

// one workgroup: thread i adds the partials of workgroups i, i + 1024, .. in that order, then a fixed tree; nparts = 0 gives 0,
// and a component whose bit of `mask` is clear is written as 0.  No float atomics anywhere: the same call gives the same bits.
template <int NC>
__global__ __launch_bounds__(1024) void tile_combine(const double* __restrict__ part, int64_t nparts, unsigned mask, float* __restrict__ res) {
    __shared__ double red[NC][1024];
    double s[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) s[c] = 0.0;
    for (int64_t i = threadIdx.x; i < nparts; i += 1024)
#pragma unroll
        for (int c = 0; c < NC; ++c) s[c] += part[NC * i + c];
#pragma unroll
    for (int c = 0; c < NC; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
#pragma unroll
            for (int c = 0; c < NC; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0)
#pragma unroll
        for (int c = 0; c < NC; ++c) res[c] = (mask >> c & 1u) ? (float)red[c][0] : 0.f;
}

}  // namespace kccot
