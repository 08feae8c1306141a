// d(loss) / d(sigma) of the kernel smoothing of smooth.hip (include/kccot_smooth_sigma.h; NOT reference behaviour: the
// reference anneals sigma by hand).  With s = A(sigma) x, m = max s, out = s / m and the upstream gradient g:
//     dsigma = sum_e u[e] * (ds/dsigma)[e],   u = g / m - [out == 1] * (sum g*out) / (m * n_ties),
//     ds/dsigma = sum_a (prod_{b != a} A_b) A'_a x          (A'_a: the stencil of axis a with the derivative taps).
// Carried through the stage order T, W, H as TWO fields, F = the smoothing so far and G = its derivative so far:
//     T:  F = K_t x,             G = K'_t x
//     W:  F <- K_w F,            G <- K'_w F + K_w G         (both from the T stage's F and G)
//     H:  ds/dsigma = K_h G + K'_h F
// An axis that is not smoothed passes both fields through.  One kernel serves every subset of the axes and the causal T stencil.
//
// dsigma_tile: a workgroup owns, of one sample, a tile of tt rows of T, wt columns of W and ct channels, and a segment of hs
// image rows, and WALKS along H as smooth_fused3 does.  Per plane: the piece with its T and W halo goes global -> LDS X (the
// borders REFLECTed on the ADDRESS: the halo is materialised, the stencils have no special cases; the piece's offsets within a
// plane are a table in LDS, built once) -> T stencil over the piece and its column halo -> LDS A (F) and A1 (G) -> W stencil at
// the owned positions (NI per thread) -> two (2R+1)-deep REGISTER windows per owned position -> H stencil -> times u, formed on
// the fly from gout / out of the plane the window completes, summed in fp64.  Two LDS barriers per plane, no intermediate in
// global memory: `in`, `gout` and `out` are read once, `in` again for the halos ((tt+2R)/tt, (wt+2R)/wt and (hs+2R)/hs of
// it; R/tt for the causal T).  Every shape finds a tiling (all three extents of the tile can shrink to 1), so there is no
// staged form.
// The sum: one fp64 partial per workgroup into the workspace, tile_combine (one workgroup, fixed order, fp64) writes the
// fp32 result.  No float atomics anywhere: the same call gives the same bits.
// What this file shares with smooth_aniso.hip lives in tile_walk.h: the tiling rule (tile_plan), the geometry of a plan
// (TileGeom), the largest-grid search behind the workspace size, REFLECT and tile_combine.
#include "common.h"
#include "smooth_internal.h"
#include "tile_walk.h"
#include "../../include/kccot_smooth_sigma.h"
#include <math.h>
#include <stdint.h>

namespace kccot {

namespace {

constexpr int DS_NT = TILE_NT;              // threads of a dsigma_tile workgroup
constexpr size_t DS_LDS_MAX = 60 * 1024;    // dynamic LDS a tiling may take (the static part is below 1 KB)
constexpr unsigned DS_AXES = KCCOT_SMOOTH_T | KCCOT_SMOOTH_H | KCCOT_SMOOTH_W;

struct DsArgs {
    const float* in;
    const float* gout;
    const float* out;
    const float* mx;        // device scalar: the maximum the forward divided by
    const float* stats;     // {sum gout*out, n_ties}
    double* part;           // one partial per workgroup
    TileGeom g;             // (an axis that is not smoothed may have been merged into its outer neighbour by the host)
    int doT, doW, doH, causal;
    SymD sd;
    CausD cd;
};

template <int R, int NI>
__global__ __launch_bounds__(DS_NT) void dsigma_tile(DsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ds_lds[];
    __shared__ float cv[SM_MAXR + 1][SM_MAXR + 1], cdv[SM_MAXR + 1][SM_MAXR + 1];
    __shared__ double wpart[DS_NT / 64];
    constexpr int NW = 2 * R + 1;
    const int tid = threadIdx.x;
    const bool doT = a.doT, doW = a.doW, doH = a.doH, causal = a.causal;
    const TileGeom& G = a.g;
    int blk = blockIdx.x;
    const int tc = blk % G.ntc; blk /= G.ntc;
    const int tw = blk % G.ntw; blk /= G.ntw;
    const int ttile = blk % G.ntt; blk /= G.ntt;
    const int seg = blk % G.nseg, b = blk / G.nseg;
    const int t0 = ttile * G.tt, w0 = tw * G.wt, c0 = tc * G.ct, h0 = seg * G.hs, h1 = min(h0 + G.hs, G.H);
    const int rw = doW ? R : 0, tbefore = doT ? R : 0, tafter = (doT && !causal) ? R : 0;
    const int ct = G.ct, pitch = (G.wt + 2 * rw) * ct, nrx = G.tt + tbefore + tafter;
    const int nx = nrx * pitch, na = G.tt * pitch;
    float* X = ds_lds;                                      // nrx x pitch: the plane piece with its halo
    int* xoff = reinterpret_cast<int*>(ds_lds + nx);        // its offsets within a plane
    float* A = ds_lds + 2 * nx;                             // tt x pitch: F behind the T stage
    float* A1 = A + na;                                     // tt x pitch: G behind the T stage
    const int64_t P = (int64_t)G.T * G.W * G.C;
    const float* inb = a.in + (int64_t)b * G.H * P;

    for (int e = tid; e < nx; e += DS_NT) {
        const int row = e / pitch, col = e - row * pitch, wc = col / ct, cc = col - wc * ct;
        int tg = t0 - tbefore + row;
        tg = causal ? (tg < 0 ? 0 : (tg > G.T - 1 ? G.T - 1 : tg)) : tile_reflect(tg, G.T);
        const int wg = tile_reflect(w0 - rw + wc, G.W), cg = min(c0 + cc, G.C - 1);
        xoff[e] = (tg * G.W + wg) * G.C + cg;
    }
    if (tid < (SM_MAXR + 1) * (SM_MAXR + 1)) {
        (&cv[0][0])[tid] = (&a.cd.v[0][0])[tid];
        (&cdv[0][0])[tid] = (&a.cd.dv[0][0])[tid];
    }
    // owned positions of the tile: fixed for the whole walk
    int aoff[NI], goff[NI];
    bool ok[NI];
    const int items = G.tt * G.wt * ct;
#pragma unroll
    for (int n = 0; n < NI; ++n) {
        int i = tid + DS_NT * n;
        const bool in_tile = i < items;
        i = in_tile ? i : 0;
        const int tr = i / (G.wt * ct), rem = i - tr * (G.wt * ct), wl = rem / ct, cl = rem - wl * ct;
        ok[n] = in_tile && t0 + tr < G.T && w0 + wl < G.W && c0 + cl < G.C;
        aoff[n] = tr * pitch + (wl + rw) * ct + cl;
        goff[n] = ok[n] ? ((t0 + tr) * G.W + w0 + wl) * G.C + c0 + cl : 0;
    }
    const float m = a.mx[0];
    const float corr = a.stats[1] > 0.f ? a.stats[0] / (m * a.stats[1]) : 0.f;
    float winF[NI][NW], winG[NI][NW];
#pragma unroll
    for (int n = 0; n < NI; ++n)
#pragma unroll
        for (int j = 0; j < NW; ++j) { winF[n][j] = 0.f; winG[n][j] = 0.f; }
    double acc = 0.0;
    const int q256 = DS_NT / pitch, r256 = DS_NT - q256 * pitch;
    const int hlo = doH ? h0 - R : h0, hhi = doH ? h1 + R : h1;
    for (int hp = hlo; hp < hhi; ++hp) {
        const int hout = doH ? hp - R : hp;         // the plane this step completes
        // its gout / out: issued first, needed last
        float gv[NI], ov[NI];
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            gv[n] = 0.f; ov[n] = 0.f;
            if (hout >= h0 && ok[n]) {
                const int64_t o = ((int64_t)b * G.H + hout) * P + goff[n];
                gv[n] = a.gout[o]; ov[n] = a.out[o];
            }
        }
        const float* inp = inb + (int64_t)tile_reflect(hp, G.H) * P;
        __syncthreads();                            // the table (first step); the T stage of the step before has read X
        for (int e = tid; e < nx; e += DS_NT) X[e] = inp[xoff[e]];
        __syncthreads();
        // ---- T stage over the piece and its column halo
        {
            int row = tid / pitch, col = tid - row * pitch;
            for (int e = tid; e < na; e += DS_NT) {
                float f, g = 0.f;
                if (!doT) f = X[e];
                else if (!causal) {
                    const float* c = X + e;         // row + R + k of X, k = -R..R
                    f = 0.f;
#pragma unroll
                    for (int k = 0; k < NW; ++k) {
                        const float x = c[k * pitch];
                        f = fmaf(a.sd.w[k], x, f); g = fmaf(a.sd.dw[k], x, g);
                    }
                } else {
                    const int tr = min(t0 + row, R);
                    const float* c = X + e + R * pitch;
                    f = 0.f;
#pragma unroll
                    for (int d = 0; d <= R; ++d) {
                        const float x = c[-d * pitch];
                        f = fmaf(cv[tr][d], x, f); g = fmaf(cdv[tr][d], x, g);
                    }
                }
                A[e] = f; A1[e] = g;
                row += q256; col += r256;
                if (col >= pitch) { col -= pitch; ++row; }
            }
        }
        __syncthreads();
        // ---- W stage at the owned positions, then the H windows
        float dsv[NI];
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            float f, g;
            if (!doW) { f = A[aoff[n]]; g = A1[aoff[n]]; }
            else {
                f = 0.f; g = 0.f;
                const float* pf = A + aoff[n] - R * ct;
                const float* pg = A1 + aoff[n] - R * ct;
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    const float x = pf[k * ct], y = pg[k * ct];
                    f = fmaf(a.sd.w[k], x, f);
                    g = fmaf(a.sd.dw[k], x, g); g = fmaf(a.sd.w[k], y, g);
                }
            }
            if (doH) {
#pragma unroll
                for (int j = 0; j < NW - 1; ++j) { winF[n][j] = winF[n][j + 1]; winG[n][j] = winG[n][j + 1]; }
                winF[n][NW - 1] = f; winG[n][NW - 1] = g;
                float d = 0.f;
#pragma unroll
                for (int j = 0; j < NW; ++j) { d = fmaf(a.sd.w[j], winG[n][j], d); d = fmaf(a.sd.dw[j], winF[n][j], d); }
                dsv[n] = d;
            } else dsv[n] = g;
        }
        if (hout < h0) continue;                    // window not full yet (uniform)
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            const float u = gv[n] / m - (ov[n] == 1.0f ? corr : 0.f);
            if (ok[n]) acc = fma((double)u, (double)dsv[n], acc);
        }
    }
    acc = wave_sum_d(acc);
    if ((tid & 63) == 0) wpart[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) a.part[blockIdx.x] = (wpart[0] + wpart[1]) + (wpart[2] + wpart[3]);
}

// ---- the tiling ----------------------------------------------------------------------------------------------------------------
struct DsShape { int B, H, T, W, C; bool doT, doW, doH, causal; };

// The kernel's view of a call: an axis that is not smoothed has no halo and no stencil, so W merges into C's place (the
// innermost run of W*C floats is one "channel" axis of a one-column image) and B into H (the walk has no window then: a
// segment is just a run of planes, and what a workgroup sets up once serves all of them).
DsShape ds_shape(int B, int H, int T, int W, int C, unsigned axes, int radius) {
    DsShape s{B, H, T, W, C, (axes & KCCOT_SMOOTH_T) && radius, (axes & KCCOT_SMOOTH_W) && radius, (axes & KCCOT_SMOOTH_H) && radius,
              (axes & KCCOT_SMOOTH_CAUSAL_T) != 0};
    if (!s.doW && (int64_t)W * C <= 0x7fffffff) { s.C = W * C; s.W = 1; }
    if (!s.doH && (int64_t)B * H <= 0x7fffffff) { s.H = B * H; s.B = 1; }      // (the walk then runs over the planes of all samples)
    return s;
}

// owned positions per thread: two windows of 2r+1 registers each, held to ~110 registers
constexpr int ds_max_ni(int radius) { return radius <= 3 ? 8 : (radius == 4 ? 6 : (radius == 5 ? 5 : 4)); }

// what tile_plan (tile_walk.h) searches for this call: the halo of every smoothed axis, two fields (F and G) behind the T stage
TileSearch ds_search(const DsShape& s, int radius) {
    const int rt = s.doT ? radius : 0;
    return TileSearch{s.B, s.H, s.T, s.W, s.C, rt, s.causal ? 0 : rt, s.doW ? radius : 0, s.doH ? radius : 0,
                      (int64_t)ds_max_ni(radius) * DS_NT, 2, DS_LDS_MAX, false};
}

// Workspace: [one fp64 partial per workgroup of the LARGEST grid any (radius, axes) plan launches at this shape]
//            [256 bytes: the two sums when the call computes them] [two per-block arrays of smooth_maxnorm_stats]
struct DsWs {
    size_t part, scal, blk, total;
    DsWs(int B, int H, int T, int W, int C) {
        static thread_local TileGridCache last{};       // (the search over every plan is a few hundred thousand steps)
        const int64_t g = tile_largest_grid(last, B, H, T, W, C, [&](auto visit) {
            for (int radius = 1; radius <= SM_MAXR; ++radius)
                for (unsigned axes = 1; axes <= DS_AXES; ++axes)
                    for (unsigned causal = 0; causal <= ((axes & KCCOT_SMOOTH_T) ? 1u : 0u); ++causal)
                        visit(tile_plan(ds_search(ds_shape(B, H, T, W, C, axes | (causal ? KCCOT_SMOOTH_CAUSAL_T : 0u), radius), radius)));
        });
        const int64_t n = (int64_t)((size_t)B * H * T * W * C);
        part = up256((size_t)g * sizeof(double));
        scal = 256;
        blk = up256((size_t)((n + 255) / 256) * sizeof(float));
        total = part + scal + 2 * blk + 256;        // (+ 256: the areas start at the next 256-byte boundary of ws)
    }
};

template <int R, int NI>
int launch_tile_ni(const TilePlan& pl, const DsArgs& a, hipStream_t st) {
    if constexpr (NI > ds_max_ni(R)) return fail(KCCOT_EUNSUPPORTED, "smooth_dsigma: no kernel for %d positions per thread at radius %d", NI, R);
    else {
        hipLaunchKernelGGL((dsigma_tile<R, NI>), dim3((unsigned)pl.grid), dim3(DS_NT), pl.lds, st, a);
        return launch_status("dsigma_tile");
    }
}

template <int R>
int launch_tile(const TilePlan& pl, const DsArgs& a, hipStream_t st) {
    switch (pl.ni) {
        case 1: return launch_tile_ni<R, 1>(pl, a, st);
        case 2: return launch_tile_ni<R, 2>(pl, a, st);
        case 3: return launch_tile_ni<R, 3>(pl, a, st);
        case 4: return launch_tile_ni<R, 4>(pl, a, st);
        case 5: return launch_tile_ni<R, 5>(pl, a, st);
        case 6: return launch_tile_ni<R, 6>(pl, a, st);
        case 7: return launch_tile_ni<R, 7>(pl, a, st);
        default: return launch_tile_ni<R, 8>(pl, a, st);
    }
}

// does this call launch dsigma_tile at all (else the result is exactly 0)
bool ds_launches(int radius, unsigned axes_flags) { return radius > 0 && (axes_flags & DS_AXES); }

// the checks of the flags; then (ds_check_dims) those of the shape and the radius.  sigma: NULL where the caller has none (the
// plan query)
int ds_check_flags(const char* who, unsigned axes_flags) {
    if (axes_flags & KCCOT_SMOOTH_NO_DIVIDE) return fail(KCCOT_EINVAL, "%s: KCCOT_SMOOTH_NO_DIVIDE is not an axis flag", who);
    if (axes_flags & KCCOT_SMOOTH_EXTERNAL_MAX) return fail(KCCOT_EINVAL, "%s: KCCOT_SMOOTH_EXTERNAL_MAX is not an axis flag", who);
    if (axes_flags & KCCOT_SMOOTH_STATS_ONLY) return fail(KCCOT_EINVAL, "%s: KCCOT_SMOOTH_STATS_ONLY is not an axis flag", who);
    if (axes_flags & KCCOT_SMOOTH_EXTERNAL_STATS)
        return fail(KCCOT_EINVAL, "%s: KCCOT_SMOOTH_EXTERNAL_STATS is not an axis flag (hand the sums in through stats_in)", who);
    if (axes_flags & ~(DS_AXES | KCCOT_SMOOTH_CAUSAL_T)) return fail(KCCOT_EINVAL, "%s: unknown flag bits 0x%x", who, axes_flags);
    if ((axes_flags & KCCOT_SMOOTH_CAUSAL_T) && !(axes_flags & KCCOT_SMOOTH_T))
        return fail(KCCOT_EINVAL, "%s: KCCOT_SMOOTH_CAUSAL_T needs KCCOT_SMOOTH_T", who);
    return 0;
}

int ds_check_dims(const char* who, int B, int H, int T, int W, int C, int radius, unsigned axes_flags, const float* sigma) {
    if (B <= 0 || H <= 0 || T <= 0 || W <= 0 || C <= 0) return fail(KCCOT_EINVAL, "%s: bad shape [%d,%d,%d,%d,%d]", who, B, H, T, W, C);
    if (radius < 0 || radius > SM_MAXR) return fail(KCCOT_EINVAL, "%s: radius %d outside 0..%d", who, radius, SM_MAXR);
    if (sigma && !(*sigma > 0.f)) return fail(KCCOT_EINVAL, "%s: sigma must be > 0", who);
    const bool causal = (axes_flags & KCCOT_SMOOTH_CAUSAL_T) != 0;
    // REFLECT padding needs pad < dim; a causal T has no padding: any radius, radius >= T included
    if (((axes_flags & KCCOT_SMOOTH_T) && !causal && radius >= T) || ((axes_flags & KCCOT_SMOOTH_H) && radius >= H) ||
        ((axes_flags & KCCOT_SMOOTH_W) && radius >= W))
        return fail(KCCOT_EINVAL, "%s: REFLECT padding needs radius < the length of every symmetric axis", who);
    return 0;
}

int ds_check_size(const char* who, int B, int H, int T, int W, int C) {
    const int64_t n = (int64_t)((size_t)B * H * T * W * C);
    if ((n + 255) / 256 > 0x7fffffff || (int64_t)T * W * C > 0x7fffffff) return fail(KCCOT_EUNSUPPORTED, "%s: tensor too large", who);
    return 0;
}

}  // namespace

}  // namespace kccot

using namespace kccot;

extern "C" int kccot_smooth_dsigma_plan(int B, int H, int T, int W, int C, int radius, unsigned axes_flags, int* out) {
    const char* who = "smooth_dsigma_plan";
    int rc;
    if ((rc = ds_check_flags(who, axes_flags))) return rc;
    if (!out) return fail(KCCOT_EINVAL, "%s: null pointer", who);
    if ((rc = ds_check_dims(who, B, H, T, W, C, radius, axes_flags, nullptr))) return rc;
    if ((rc = ds_check_size(who, B, H, T, W, C))) return rc;
    for (int k = 0; k < KCCOT_SMOOTH_DSIGMA_PLAN_INTS; ++k) out[k] = 0;
    if (!ds_launches(radius, axes_flags)) return 0;
    const DsShape s = ds_shape(B, H, T, W, C, axes_flags, radius);
    const TileSearch q = ds_search(s, radius);
    const TilePlan pl = tile_plan(q);
    if (!pl.ok) return fail(KCCOT_EUNSUPPORTED, "%s: no tiling for [%d,%d,%d,%d,%d] at radius %d", who, B, H, T, W, C, radius);
    const TileGeom g = tile_geometry(q, pl);
    const int v[KCCOT_SMOOTH_DSIGMA_PLAN_INTS] = {1, radius, pl.ni, g.tt, g.wt, g.ct, g.hs, g.ntt, g.ntw, g.ntc, g.nseg, (int)pl.grid,
                                                  s.B, g.H, g.T, g.W, g.C};
    for (int k = 0; k < KCCOT_SMOOTH_DSIGMA_PLAN_INTS; ++k) out[k] = v[k];
    return 0;
}

extern "C" size_t kccot_smooth_dsigma_workspace_bytes(int B, int H, int T, int W, int C) {
    if (B <= 0 || H <= 0 || T <= 0 || W <= 0 || C <= 0) return 0;
    return DsWs(B, H, T, W, C).total;
}

extern "C" int kccot_smooth_dsigma_f32(const float* in, const float* gout, const float* out, const float* max_in,
                                       const float* stats_in, int B, int H, int T, int W, int C, float sigma, int radius,
                                       unsigned axes_flags, float* dsigma_out, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const char* who = "smooth_dsigma";
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = ds_check_flags(who, axes_flags))) return rc;
    if (!in || !gout || !out || !max_in || !dsigma_out) return fail(KCCOT_EINVAL, "%s: null pointer", who);
    if ((rc = ds_check_dims(who, B, H, T, W, C, radius, axes_flags, &sigma))) return rc;
    const DsWs lay(B, H, T, W, C);
    if (!ws || ws_bytes < lay.total) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", who, ws_bytes, lay.total);
    if ((rc = ds_check_size(who, B, H, T, W, C))) return rc;
    const int64_t n = (int64_t)((size_t)B * H * T * W * C);

    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    double* part = reinterpret_cast<double*>(base);
    float* scal = reinterpret_cast<float*>(base + lay.part);
    float* pdot = reinterpret_cast<float*>(base + lay.part + lay.scal);
    float* pcnt = reinterpret_cast<float*>(base + lay.part + lay.scal + lay.blk);

    int64_t nparts = 0;
    if (ds_launches(radius, axes_flags)) {
        const float* stats = stats_in;
        if (!stats) {
            if ((rc = smooth_maxnorm_stats(gout, out, n, pdot, pcnt, scal, st))) return rc;
            stats = scal;
        }
        const DsShape s = ds_shape(B, H, T, W, C, axes_flags, radius);
        const TileSearch q = ds_search(s, radius);
        const TilePlan pl = tile_plan(q);
        if (!pl.ok || (size_t)pl.grid * sizeof(double) > lay.part)      // (the layout was sized from this very plan)
            return fail(KCCOT_EUNSUPPORTED, "%s: no tiling for [%d,%d,%d,%d,%d] at radius %d", who, B, H, T, W, C, radius);
        DsArgs a{};
        a.in = in; a.gout = gout; a.out = out; a.mx = max_in; a.stats = stats; a.part = part;
        a.g = tile_geometry(q, pl);
        a.doT = s.doT; a.doW = s.doW; a.doH = s.doH; a.causal = s.causal;
        a.sd = make_sym_d(sigma, radius);
        if (s.causal) a.cd = make_caus_d(sigma, radius);
        switch (radius) {
            case 1: rc = launch_tile<1>(pl, a, st); break;
            case 2: rc = launch_tile<2>(pl, a, st); break;
            case 3: rc = launch_tile<3>(pl, a, st); break;
            case 4: rc = launch_tile<4>(pl, a, st); break;
            case 5: rc = launch_tile<5>(pl, a, st); break;
            case 6: rc = launch_tile<6>(pl, a, st); break;
            default: rc = launch_tile<7>(pl, a, st); break;
        }
        if (rc) return rc;
        nparts = pl.grid;
    }
    hipLaunchKernelGGL(tile_combine<1>, dim3(1), dim3(1024), 0, st, (const double*)part, nparts, 1u, dsigma_out);
    return launch_status("tile_combine");
}
