// The anisotropic 3-D kernel smoothing (include/kccot_smooth_aniso.h; NOT reference behaviour: the reference has one sigma and
// one radius for all three axes): s = A_h(sigma_s, r_s) A_w(sigma_s, r_s) A_t(sigma_t, r_t) x, out = s / max s, its adjoint and
// the two bandwidth gradients.  Nothing here goes through the dispatch ladder of smooth.hip.
//
// aniso_tile: ONE tile walk (the one of dsigma_tile, smooth_sigma.hip; what the two files share -- the tiling rule tile_plan, the
// geometry of a plan, the largest-grid search behind the workspace size, REFLECT and tile_combine -- lives in tile_walk.h)
// serves the three jobs.  A workgroup owns, of one sample, a tile of tt rows of T, wt columns of W and ct channels, and a
// segment of hs image rows, and walks along H.  Per plane: the
// piece with its T and W halo goes global -> LDS X (through a table of offsets within a plane, built once) -> T stencil over
// the piece and its column halo (r_t is a run-time argument: this stage reads LDS only) -> LDS A -> W stencil at the owned
// positions (NI per thread) -> (2 RS + 1)-deep REGISTER windows per owned position -> H stencil -> the job's epilogue.  RS, the
// spatial radius, is a template argument because of the windows.  Every stencil is "tap table row x window": the row of the
// table is a function of the output position (an_row), so the jobs differ in tables, in what the halo holds, and in the
// epilogue:
//   JOB_FWD   halo = x on REFLECTed addresses (clamped for the causal T); uniform tables (the causal T: row min(t, r_t));
//             writes s and one block maximum per workgroup.  The host then reduces the maxima and divides `out` IN PLACE:
//             the float that is divided is the float whose maximum was taken, so the arg-max element is exactly 1.
//   JOB_ADJ   the operators of different axes commute, so din = A_t^T A_w^T A_h^T u runs in the same T -> W -> H order as a
//             GATHER: halo = u inside the tensor (formed on the fly from gout, out, m and the two batch sums), ZERO outside;
//             border rows of a REFLECT axis have tap rows of their own (the coefficients are in the header), the interior is
//             the plain stencil; the causal T gathers forwards in time with the taps v_{p+d,d}.
//   JOB_DSIG  three fields, F (smoothed so far), G_t and G_s (differentiated once along T / along H|W):
//                 T:  F = K_t x, G_t = K'_t x          W:  G_s = K'_w F, F <- K_w F, G_t <- K_w G_t
//                 H:  dsigma_t element = K_h G_t,      dsigma_s element = K_h G_s + K'_h F
//             each times u, summed in fp64 per thread; two fp64 partials per workgroup, combined by tile_combine (one
//             workgroup, fixed order).  No float atomics anywhere: the same call gives the same bits.
// Every shape and every (r_t, r_s) in 0..7 x 0..7 finds a tiling (all extents of the tile can shrink to 1): no staged form.
#include "common.h"
#include "smooth_internal.h"
#include "tile_walk.h"
#include "../../include/kccot_smooth_aniso.h"
#include <float.h>
#include <math.h>
#include <stdint.h>

namespace kccot {

namespace {

constexpr int AN_NT = TILE_NT;              // threads of an aniso_tile workgroup
constexpr size_t AN_LDS_MAX = 56 * 1024;    // dynamic LDS a tiling may take (the static part is 3.2 KB)
constexpr int AN_TW = 2 * SM_MAXR + 1;      // taps of a table row; the centre tap sits at SM_MAXR
constexpr int AN_TR = 2 * SM_MAXR + 3;      // rows of a table
enum { JOB_FWD = 0, JOB_ADJ = 1, JOB_DSIG = 2 };
enum { ROW_UNIFORM = 0, ROW_HEAD = 1, ROW_BORDER = 2 };
enum { HALO_REFLECT = 0, HALO_CLAMP = 1, HALO_ZERO = 2 };

struct AxTab { float t[AN_TR][AN_TW]; };

// Which row of an axis table serves output position p (0 <= p < L) of an axis with radius r:
//   ROW_UNIFORM  one row;   ROW_HEAD  rows 0..r for p = 0..r, row r behind (the causal T, forward and adjoint);
//   ROW_BORDER   the REFLECT adjoint: p <= r -> p, p >= L-1-r -> r+1 + (L-1-p), the interior -> 2r+2; an axis with no
//                interior (L <= 2r+2 <= 16) has a row per position.
__host__ __device__ __forceinline__ int an_row(int p, int L, int r, int kind) {
    if (kind == ROW_UNIFORM) return 0;
    p = p < 0 ? 0 : (p > L - 1 ? L - 1 : p);        // (positions only a masked output of a ragged tile asks for)
    if (kind == ROW_HEAD) return p < r ? p : r;
    if (L <= 2 * r + 2) return p;
    if (p <= r) return p;
    if (p >= L - 1 - r) return r + 1 + (L - 1 - p);
    return 2 * r + 2;
}

// every row = the symmetric taps w[0..2r] (centre r)
AxTab tab_uniform(const float* w, int r) {
    AxTab a{};
    for (int k = -r; k <= r; ++k) a.t[0][SM_MAXR + k] = w[k + r];
    return a;
}

// causal forward: row t holds v[t][d] at offset -d
AxTab tab_causal_fwd(const float v[SM_MAXR + 1][SM_MAXR + 1], int r) {
    AxTab a{};
    for (int t = 0; t <= r; ++t)
        for (int d = 0; d <= t; ++d) a.t[t][SM_MAXR - d] = v[t][d];
    return a;
}

// causal adjoint: din[p] = sum_d v_{p+d,d} u[p+d]; row min(p, r) holds v[min(p+d, r)][d] at offset +d (u is zero behind T-1)
AxTab tab_causal_adj(const float v[SM_MAXR + 1][SM_MAXR + 1], int r) {
    AxTab a{};
    for (int p = 0; p <= r; ++p)
        for (int d = 0; d <= r; ++d) a.t[p][SM_MAXR + d] = v[p + d < r ? p + d : r][d];
    return a;
}

// REFLECT adjoint on an axis of length L > r: the coefficient of u[q] in din[p] (the derivation is in the header)
AxTab tab_reflect_adj(const float* w, int r, int L) {
    AxTab a{};
    auto W = [&](int d) { return w[d + r]; };
    auto fill = [&](int p) {
        float* row = a.t[an_row(p, L, r, ROW_BORDER)];
        for (int k = -r; k <= r; ++k) {
            const int q = p + k;
            float c = 0.f;
            if (q >= 0 && q < L) {
                c = W(q - p);
                if (p >= 1 && p + q <= r) c += W(p + q);
                if (p <= L - 2 && (L - 1 - p) + (L - 1 - q) <= r) c += W(2 * (L - 1) - p - q);
            }
            row[SM_MAXR + k] = c;
        }
    };
    if (L <= 2 * r + 2) { for (int p = 0; p < L; ++p) fill(p); }
    else {
        for (int p = 0; p <= r; ++p) { fill(p); fill(L - 1 - p); }
        fill(r + 1);                                // an interior position: the plain stencil
    }
    return a;
}

struct AnArgs {
    const float* in;        // JOB_FWD / JOB_DSIG: x
    const float* gout;      // JOB_ADJ / JOB_DSIG
    const float* outf;      // JOB_ADJ / JOB_DSIG: the forward's out
    const float* mx;        // device scalar: the maximum the forward divided by
    const float* stats;     // {sum gout*out, n_ties}
    float* res;             // JOB_FWD: s; JOB_ADJ: din
    float* bmax;            // JOB_FWD: one maximum per workgroup
    double* part;           // JOB_DSIG: two partials per workgroup
    TileGeom g;
    int rt, tb, ta;         // T radius; halo rows before / after the piece
    int kind_t, halo_t;     // ROW_* of the T table; HALO_* of the T halo (W and H: REFLECT, JOB_ADJ: ZERO)
    float ws[AN_TW], dws[AN_TW];    // JOB_FWD / JOB_DSIG: the uniform spatial taps (centre RS) and their derivative
    AxTab tab[3];           // [0] T;  [1] JOB_DSIG: the derivative T table, JOB_ADJ: W;  [2] JOB_ADJ: H
};

template <int RS, int NI, int JOB>
__global__ __launch_bounds__(AN_NT) void aniso_tile(AnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float an_lds[];
    __shared__ float tabs[3][AN_TR * AN_TW];
    __shared__ float red[16];
    __shared__ double wpart[2][AN_NT / 64];
    constexpr int NW = 2 * RS + 1;
    constexpr bool ADJ = JOB == JOB_ADJ, DSIG = JOB == JOB_DSIG;
    const int tid = threadIdx.x;
    const TileGeom& G = a.g;
    int blk = blockIdx.x;
    const int tc = blk % G.ntc; blk /= G.ntc;
    const int tw = blk % G.ntw; blk /= G.ntw;
    const int ttile = blk % G.ntt; blk /= G.ntt;
    const int seg = blk % G.nseg, b = blk / G.nseg;
    const int t0 = ttile * G.tt, w0 = tw * G.wt, c0 = tc * G.ct, h0 = seg * G.hs, h1 = min(h0 + G.hs, G.H);
    const int tb = a.tb, ta = a.ta, ct = G.ct, pitch = (G.wt + 2 * RS) * ct, nrx = G.tt + tb + ta;
    const int nx = nrx * pitch, na = G.tt * pitch;
    float* X = an_lds;                                      // nrx x pitch: the plane piece with its halo
    int* xoff = reinterpret_cast<int*>(an_lds + nx);        // its offsets within a plane; -1 = outside the tensor (JOB_ADJ)
    float* A = an_lds + 2 * nx;                             // tt x pitch: F behind the T stage
    float* A1 = A + na;                                     // tt x pitch: G_t behind the T stage (JOB_DSIG)
    const int64_t P = (int64_t)G.T * G.W * G.C;

    for (int e = tid; e < nx; e += AN_NT) {
        const int row = e / pitch, col = e - row * pitch, wc = col / ct, cc = col - wc * ct;
        const int traw = t0 - tb + row, wraw = w0 - RS + wc;
        int tg, wg;
        bool inside = true;
        if (a.halo_t == HALO_REFLECT) tg = tile_reflect(traw, G.T);
        else {
            inside = traw >= 0 && traw < G.T;
            tg = traw < 0 ? 0 : (traw > G.T - 1 ? G.T - 1 : traw);
        }
        if (ADJ) { inside = inside && wraw >= 0 && wraw < G.W; wg = inside ? wraw : 0; }
        else wg = tile_reflect(wraw, G.W);
        const int cg = min(c0 + cc, G.C - 1);
        xoff[e] = (ADJ && !inside) ? -1 : (tg * G.W + wg) * G.C + cg;
    }
    for (int i = tid; i < AN_TR * AN_TW; i += AN_NT) {
        tabs[0][i] = (&a.tab[0].t[0][0])[i];
        if (ADJ || DSIG) tabs[1][i] = (&a.tab[1].t[0][0])[i];
        if (ADJ) tabs[2][i] = (&a.tab[2].t[0][0])[i];
    }
    // owned positions of the tile: fixed for the whole walk
    int aoff[NI], goff[NI], roww[NI];
    bool ok[NI];
    const int items = G.tt * G.wt * ct;
#pragma unroll
    for (int n = 0; n < NI; ++n) {
        int i = tid + AN_NT * n;
        const bool in_tile = i < items;
        i = in_tile ? i : 0;
        const int tr = i / (G.wt * ct), rem = i - tr * (G.wt * ct), wl = rem / ct, cl = rem - wl * ct;
        ok[n] = in_tile && t0 + tr < G.T && w0 + wl < G.W && c0 + cl < G.C;
        aoff[n] = tr * pitch + (wl + RS) * ct + cl;
        goff[n] = ok[n] ? ((t0 + tr) * G.W + w0 + wl) * G.C + c0 + cl : 0;
        roww[n] = ADJ ? an_row(w0 + wl, G.W, RS, ROW_BORDER) * AN_TW + SM_MAXR : 0;
    }
    float m = 1.f, corr = 0.f;
    if (ADJ || DSIG) {
        m = a.mx[0];
        corr = a.stats[1] > 0.f ? a.stats[0] / (m * a.stats[1]) : 0.f;
    }
    float winF[NI][NW], winT[DSIG ? NI : 1][NW], winS[DSIG ? NI : 1][NW];
#pragma unroll
    for (int n = 0; n < NI; ++n)
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            winF[n][j] = 0.f;
            if (DSIG) { winT[n][j] = 0.f; winS[n][j] = 0.f; }
        }
    double acc_t = 0.0, acc_s = 0.0;
    float vmax = -FLT_MAX;
    const int q256 = AN_NT / pitch, r256 = AN_NT - q256 * pitch;
    const int ntaps = tb + ta + 1, tap0 = SM_MAXR - tb;
    const int64_t sample = (int64_t)b * G.H * P;
    for (int hp = h0 - RS; hp < h1 + RS; ++hp) {
        const int hout = hp - RS;                   // the plane this step completes
        // JOB_DSIG: its gout / out, issued first, needed last
        float gv[DSIG ? NI : 1], ov[DSIG ? NI : 1];
        if (DSIG) {
#pragma unroll
            for (int n = 0; n < NI; ++n) {
                gv[n] = 0.f; ov[n] = 0.f;
                if (hout >= h0 && ok[n]) {
                    const int64_t o = sample + (int64_t)hout * P + goff[n];
                    gv[n] = a.gout[o]; ov[n] = a.outf[o];
                }
            }
        }
        const bool plane = !ADJ || (hp >= 0 && hp < G.H);       // JOB_ADJ: u is zero outside the tensor (uniform)
        float fv[NI], tv[DSIG ? NI : 1], sv[DSIG ? NI : 1];
        if (plane) {
            const int64_t base = sample + (int64_t)(ADJ ? hp : tile_reflect(hp, G.H)) * P;
            __syncthreads();                        // the tables (first step); the T stage of the step before has read X
            if (ADJ) {
                const float* gp = a.gout + base;
                const float* op = a.outf + base;
                for (int e = tid; e < nx; e += AN_NT) {
                    const int o = xoff[e];
                    X[e] = o < 0 ? 0.f : gp[o] / m - (op[o] == 1.0f ? corr : 0.f);
                }
            } else {
                const float* inp = a.in + base;
                for (int e = tid; e < nx; e += AN_NT) X[e] = inp[xoff[e]];
            }
            __syncthreads();
            // ---- T stage over the piece and its column halo
            {
                int row = tid / pitch, col = tid - row * pitch;
                for (int e = tid; e < na; e += AN_NT) {
                    const int tr = an_row(t0 + row, G.T, a.rt, a.kind_t) * AN_TW + tap0;
                    const float* c = X + e;
                    float f = 0.f, g = 0.f;
                    for (int k = 0; k < ntaps; ++k) {
                        const float x = c[k * pitch];
                        f = fmaf(tabs[0][tr + k], x, f);
                        if (DSIG) g = fmaf(tabs[1][tr + k], x, g);
                    }
                    A[e] = f;
                    if (DSIG) A1[e] = g;
                    row += q256; col += r256;
                    if (col >= pitch) { col -= pitch; ++row; }
                }
            }
            __syncthreads();
            // ---- W stage at the owned positions
#pragma unroll
            for (int n = 0; n < NI; ++n) {
                float f = 0.f, gt = 0.f, gs = 0.f;
                if constexpr (RS == 0) {
                    f = A[aoff[n]];
                    if (DSIG) gt = A1[aoff[n]];
                } else {
                    const float* pf = A + aoff[n] - RS * ct;
                    const float* pg = A1 + aoff[n] - RS * ct;
#pragma unroll
                    for (int k = 0; k < NW; ++k) {
                        const float x = pf[k * ct];
                        if (ADJ) f = fmaf(tabs[1][roww[n] - RS + k], x, f);
                        else f = fmaf(a.ws[k], x, f);
                        if (DSIG) { gs = fmaf(a.dws[k], x, gs); gt = fmaf(a.ws[k], pg[k * ct], gt); }
                    }
                }
                fv[n] = f;
                if (DSIG) { tv[n] = gt; sv[n] = gs; }
            }
        } else {
#pragma unroll
            for (int n = 0; n < NI; ++n) fv[n] = 0.f;
        }
        // ---- the H windows and the H stencil
        const int rowh = ADJ ? an_row(hout, G.H, RS, ROW_BORDER) * AN_TW + SM_MAXR - RS : 0;
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            if constexpr (RS > 0) {
#pragma unroll
                for (int j = 0; j < NW - 1; ++j) {
                    winF[n][j] = winF[n][j + 1];
                    if (DSIG) { winT[n][j] = winT[n][j + 1]; winS[n][j] = winS[n][j + 1]; }
                }
                winF[n][NW - 1] = fv[n];
                if (DSIG) { winT[n][NW - 1] = tv[n]; winS[n][NW - 1] = sv[n]; }
                float f = 0.f, dt = 0.f, ds = 0.f;
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    if (ADJ) f = fmaf(tabs[2][rowh + j], winF[n][j], f);
                    else if (!DSIG) f = fmaf(a.ws[j], winF[n][j], f);
                    if (DSIG) {
                        dt = fmaf(a.ws[j], winT[n][j], dt);
                        ds = fmaf(a.ws[j], winS[n][j], ds); ds = fmaf(a.dws[j], winF[n][j], ds);
                    }
                }
                fv[n] = f;
                if (DSIG) { tv[n] = dt; sv[n] = ds; }
            }
        }
        if (hout < h0) continue;                    // window not full yet (uniform)
#pragma unroll
        for (int n = 0; n < NI; ++n) {
            if (!ok[n]) continue;
            if (DSIG) {
                const float u = gv[n] / m - (ov[n] == 1.0f ? corr : 0.f);
                acc_t = fma((double)u, (double)tv[n], acc_t);
                acc_s = fma((double)u, (double)sv[n], acc_s);
            } else {
                a.res[sample + (int64_t)hout * P + goff[n]] = fv[n];
                if (!ADJ) vmax = fmaxf(vmax, fv[n]);
            }
        }
    }
    if (JOB == JOB_FWD) {
        const float bm = block_max(vmax, red);
        if (tid == 0) a.bmax[blockIdx.x] = bm;
    }
    if (DSIG) {
        acc_t = wave_sum_d(acc_t);
        acc_s = wave_sum_d(acc_s);
        if ((tid & 63) == 0) { wpart[0][tid >> 6] = acc_t; wpart[1][tid >> 6] = acc_s; }
        __syncthreads();
        if (tid < 2) a.part[2 * (int64_t)blockIdx.x + tid] = (wpart[tid][0] + wpart[tid][1]) + (wpart[tid][2] + wpart[tid][3]);
    }
}

__global__ __launch_bounds__(1024) void aniso_reduce_max(const float* __restrict__ bmax, int64_t nb, float* __restrict__ mx) {
    __shared__ float red[16];
    float m = -FLT_MAX;
    for (int64_t i = threadIdx.x; i < nb; i += 1024) m = fmaxf(m, bmax[i]);
    m = block_max(m, red);
    if (threadIdx.x == 0) mx[0] = m;
}

__global__ __launch_bounds__(256) void aniso_divide(float* __restrict__ out, int64_t n, const float* __restrict__ mx) {
    const float m = mx[0];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) out[e] = out[e] / m;
}

// The two batch sums of the normalisation's adjoint, {sum gout*out, #(out == 1)}, taken PER SAMPLE and then added over the
// samples in fp32 in sample order.  smooth_maxnorm_stats cuts the flat tensor into blocks that straddle samples and rounds once
// at the end, so the sums of two shards added on the host differ from its one-call sum in the last bit, and with them every din
// near an arg-max element.  Here a shard of one sample hands back exactly the term the one-call sum adds for that sample: shards
// of one sample each, re-added in sample order (two shards: in either order), reproduce the one-call sums, and so din, bit for
// bit.  Three launches: 1024 elements of one sample per workgroup; one workgroup per sample (thread i adds partials i, i + 256,
// .. in fp64, then a fixed tree); one workgroup that adds the samples in order.
constexpr int AN_SB = 1024;     // elements of a sample per workgroup of the first stage

__global__ __launch_bounds__(256) void aniso_stats_partial(const float* __restrict__ gout, const float* __restrict__ out, int64_t S,
                                                           int bps, float* __restrict__ pdot, float* __restrict__ pcnt) {
    __shared__ float red[16];
    const int64_t b = blockIdx.x / bps, k = blockIdx.x % bps, base = b * S;
    float d = 0.f, c = 0.f;
#pragma unroll
    for (int j = 0; j < AN_SB / 256; ++j) {
        const int64_t e = k * AN_SB + j * 256 + threadIdx.x;
        if (e < S) {
            const float o = out[base + e];
            d = fmaf(gout[base + e], o, d);
            c += o == 1.0f ? 1.f : 0.f;
        }
    }
    d = block_sum(d, red);
    c = block_sum(c, red);
    if (threadIdx.x == 0) { pdot[blockIdx.x] = d; pcnt[blockIdx.x] = c; }
}

__global__ __launch_bounds__(256) void aniso_stats_sample(const float* __restrict__ pdot, const float* __restrict__ pcnt, int bps,
                                                          float* __restrict__ sdot, float* __restrict__ scnt) {
    __shared__ double rd[256];
    __shared__ float rc[256];
    const int64_t base = (int64_t)blockIdx.x * bps;
    double d = 0.0;
    float c = 0.f;
    for (int k = threadIdx.x; k < bps; k += 256) { d += (double)pdot[base + k]; c += pcnt[base + k]; }
    rd[threadIdx.x] = d; rc[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) { rd[threadIdx.x] += rd[threadIdx.x + w]; rc[threadIdx.x] += rc[threadIdx.x + w]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { sdot[blockIdx.x] = (float)rd[0]; scnt[blockIdx.x] = rc[0]; }
}

__global__ __launch_bounds__(256) void aniso_stats_total(const float* __restrict__ sdot, const float* __restrict__ scnt, int B,
                                                         float* __restrict__ res) {
    __shared__ float ld[256], lc[256];
    float d = 0.f, c = 0.f;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int nb = min(256, B - b0);
        if ((int)threadIdx.x < nb) { ld[threadIdx.x] = sdot[b0 + threadIdx.x]; lc[threadIdx.x] = scnt[b0 + threadIdx.x]; }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < nb; ++i) { d += ld[i]; c += lc[i]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { res[0] = d; res[1] = c; }
}

// ---- the tiling ----------------------------------------------------------------------------------------------------------------
// owned positions per thread, one of 1, 2, 4, 8: a position costs a window of 2 rs + 1 registers, JOB_DSIG three of them, so
// NI falls as rs grows (JOB_DSIG: 3 NI (2 rs + 1) <= 90; JOB_FWD: NI (2 rs + 1) <= 60).  JOB_ADJ keeps JOB_DSIG's limits: with
// 8 positions at rs = 3 (a per-position tap row and two loads per halo element on top of the window) it measured 1.5 times
// SLOWER at configs[3] than with 4.
constexpr int an_max_ni(int rs, int job) { return job == JOB_FWD ? (rs <= 3 ? 8 : 4) : (rs <= 1 ? 8 : (rs <= 3 ? 4 : 2)); }

// what tile_plan (tile_walk.h) searches for a job: the raw shape; the halo rows of T symmetric both sides, causal behind the
// piece (forward, dsigma) or ahead of it (adjoint); a second field behind the T stage for JOB_DSIG
TileSearch an_search(int B, int H, int T, int W, int C, int rt, int rs, bool causal, int job) {
    const int tb = causal ? (job == JOB_ADJ ? 0 : rt) : rt, ta = causal ? (job == JOB_ADJ ? rt : 0) : rt;
    return TileSearch{B, H, T, W, C, tb, ta, rs, rs, (int64_t)an_max_ni(rs, job) * AN_NT, job == JOB_DSIG ? 2 : 1, AN_LDS_MAX, true};
}

// Workspace: [16 bytes per workgroup of the LARGEST grid any (job, r_t, r_s, causal) plan launches at this shape: the block
//            maxima of the forward or the two fp64 partials of dsigma] [256 bytes: the two sums when the call computes them]
//            [two arrays of one float per 1024 elements of a sample, two of one float per sample: the stages of the sums].
// The launch checks its grid against the first area again.
struct AnWs {
    size_t part, scal, blk, smp, total;
    int bps;        // workgroups per sample of aniso_stats_partial
    AnWs(int B, int H, int T, int W, int C) {
        static thread_local TileGridCache last{};       // (the search over every plan is about a million steps)
        const int64_t g = tile_largest_grid(last, B, H, T, W, C, [&](auto visit) {
            for (int job = JOB_FWD; job <= JOB_DSIG; ++job)
                for (int rt = 0; rt <= SM_MAXR; ++rt)
                    for (int rs = 0; rs <= SM_MAXR; ++rs)
                        for (int causal = 0; causal <= 1; ++causal) visit(tile_plan(an_search(B, H, T, W, C, rt, rs, causal != 0, job)));
        });
        const int64_t n = (int64_t)((size_t)B * H * T * W * C);
        part = up256((size_t)g * 2 * sizeof(double));
        scal = 256;
        const int64_t S = n / B;
        bps = (int)((S + AN_SB - 1) / AN_SB);
        blk = up256((size_t)B * bps * sizeof(float));
        smp = up256((size_t)B * sizeof(float));
        total = part + scal + 2 * blk + 2 * smp + 256;      // (+ 256: the areas start at the next 256-byte boundary of ws)
    }
};

template <int RS, int NI, int JOB>
int launch_tile_job(const TilePlan& pl, const AnArgs& a, hipStream_t st) {
    if constexpr (NI > an_max_ni(RS, JOB)) return fail(KCCOT_EUNSUPPORTED, "smooth_aniso: no kernel for %d positions per thread at radius_s %d", NI, RS);
    else {
        hipLaunchKernelGGL((aniso_tile<RS, NI, JOB>), dim3((unsigned)pl.grid), dim3(AN_NT), pl.lds, st, a);
        return launch_status("aniso_tile");
    }
}

template <int RS, int NI>
int launch_tile_ni(int job, const TilePlan& pl, const AnArgs& a, hipStream_t st) {
    if (job == JOB_FWD) return launch_tile_job<RS, NI, JOB_FWD>(pl, a, st);
    if (job == JOB_ADJ) return launch_tile_job<RS, NI, JOB_ADJ>(pl, a, st);
    return launch_tile_job<RS, NI, JOB_DSIG>(pl, a, st);
}

template <int RS>
int launch_tile_rs(int job, const TilePlan& pl, const AnArgs& a, hipStream_t st) {
    switch (pl.ni) {
        case 1: return launch_tile_ni<RS, 1>(job, pl, a, st);
        case 2: return launch_tile_ni<RS, 2>(job, pl, a, st);
        case 4: return launch_tile_ni<RS, 4>(job, pl, a, st);
        default: return launch_tile_ni<RS, 8>(job, pl, a, st);
    }
}

struct AnCall {
    const char* who;
    int B, H, T, W, C;
    float sigma_t, sigma_s;
    int rt, rs;
    unsigned flags;
    void* ws;
    size_t ws_bytes;
    hipStream_t st;
    bool causal() const { return (flags & KCCOT_SMOOTH_CAUSAL_T) != 0; }
    int64_t n() const { return (int64_t)((size_t)B * H * T * W * C); }
};

// the areas of the workspace
struct AnAreas {
    AnWs lay;
    char* base;
    AnAreas(const AnCall& c) : lay(c.B, c.H, c.T, c.W, c.C), base(reinterpret_cast<char*>(((uintptr_t)c.ws + 255) & ~(uintptr_t)255)) {}
    float* bmax() const { return reinterpret_cast<float*>(base); }
    double* part() const { return reinterpret_cast<double*>(base); }
    float* scal() const { return reinterpret_cast<float*>(base + lay.part); }
    float* pdot() const { return reinterpret_cast<float*>(base + lay.part + lay.scal); }
    float* pcnt() const { return reinterpret_cast<float*>(base + lay.part + lay.scal + lay.blk); }
    float* sdot() const { return reinterpret_cast<float*>(base + lay.part + lay.scal + 2 * lay.blk); }
    float* scnt() const { return reinterpret_cast<float*>(base + lay.part + lay.scal + 2 * lay.blk + lay.smp); }
};

// res[0..1] = the two batch sums of this call's tensor (see aniso_stats_partial)
int an_stats(const AnCall& c, const float* gout, const float* out, const AnAreas& w, float* res) {
    int rc;
    const int64_t S = c.n() / c.B;
    hipLaunchKernelGGL(aniso_stats_partial, dim3((unsigned)((int64_t)c.B * w.lay.bps)), dim3(256), 0, c.st, gout, out, S, w.lay.bps,
                       w.pdot(), w.pcnt());
    if ((rc = launch_status("aniso_stats_partial"))) return rc;
    hipLaunchKernelGGL(aniso_stats_sample, dim3((unsigned)c.B), dim3(256), 0, c.st, (const float*)w.pdot(), (const float*)w.pcnt(),
                       w.lay.bps, w.sdot(), w.scnt());
    if ((rc = launch_status("aniso_stats_sample"))) return rc;
    hipLaunchKernelGGL(aniso_stats_total, dim3(1), dim3(256), 0, c.st, (const float*)w.sdot(), (const float*)w.scnt(), c.B, res);
    return launch_status("aniso_stats_total");
}

// `allowed` = the bits this entry point takes; a refused one is named
int an_check_flags(const AnCall& c, unsigned allowed) {
    static const struct { unsigned bit; const char* name; } names[] = {
        {KCCOT_SMOOTH_T, "KCCOT_SMOOTH_T"}, {KCCOT_SMOOTH_H, "KCCOT_SMOOTH_H"}, {KCCOT_SMOOTH_W, "KCCOT_SMOOTH_W"},
        {KCCOT_SMOOTH_NO_DIVIDE, "KCCOT_SMOOTH_NO_DIVIDE"}, {KCCOT_SMOOTH_EXTERNAL_MAX, "KCCOT_SMOOTH_EXTERNAL_MAX"},
        {KCCOT_SMOOTH_STATS_ONLY, "KCCOT_SMOOTH_STATS_ONLY"}, {KCCOT_SMOOTH_EXTERNAL_STATS, "KCCOT_SMOOTH_EXTERNAL_STATS"}};
    for (const auto& f : names)
        if ((c.flags & f.bit) && !(allowed & f.bit))
            return fail(KCCOT_EINVAL, "%s: %s is not accepted here (the axes are fixed: T, H and W)", c.who, f.name);
    if (c.flags & ~(allowed | 0xffu)) return fail(KCCOT_EINVAL, "%s: unknown flag bits 0x%x", c.who, c.flags & ~(allowed | 0xffu));
    return 0;
}

// flags first, then the arguments every entry point shares
int an_check(const AnCall& c, unsigned allowed) {
    const int rc = an_check_flags(c, allowed);
    if (rc) return rc;
    if (c.B <= 0 || c.H <= 0 || c.T <= 0 || c.W <= 0 || c.C <= 0)
        return fail(KCCOT_EINVAL, "%s: bad shape [%d,%d,%d,%d,%d]", c.who, c.B, c.H, c.T, c.W, c.C);
    if (!(c.sigma_t > 0.f) || !(c.sigma_s > 0.f)) return fail(KCCOT_EINVAL, "%s: sigma_t and sigma_s must be > 0", c.who);
    if (c.rt < 0 || c.rt > SM_MAXR || c.rs < 0 || c.rs > SM_MAXR)
        return fail(KCCOT_EINVAL, "%s: radius (%d, %d) outside 0..%d", c.who, c.rt, c.rs, SM_MAXR);
    // REFLECT padding needs pad < dim; a causal T has no padding: any radius_t, radius_t >= T included
    if ((!c.causal() && c.rt >= c.T) || c.rs >= c.H || c.rs >= c.W)
        return fail(KCCOT_EINVAL, "%s: REFLECT padding needs radius < the length of every symmetric axis", c.who);
    return 0;
}

int an_check_size(const AnCall& c) {
    if ((c.n() + 255) / 256 > 0x7fffffff || (int64_t)c.T * c.W * c.C > 0x7fffffff ||
        (int64_t)c.B * ((c.n() / c.B + AN_SB - 1) / AN_SB) > 0x7fffffff) return fail(KCCOT_EUNSUPPORTED, "%s: tensor too large", c.who);
    return 0;
}

int an_check_ws(const AnCall& c) {
    const size_t need = AnWs(c.B, c.H, c.T, c.W, c.C).total;
    if (!c.ws || c.ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", c.who, c.ws_bytes, need);
    return an_check_size(c);
}

// the flag bits the entry points of a job take (`sharded`: the two-call backward)
unsigned an_allowed(int job, bool sharded = false) {
    if (job == JOB_FWD) return KCCOT_SMOOTH_CAUSAL_T | KCCOT_SMOOTH_NO_DIVIDE | KCCOT_SMOOTH_EXTERNAL_MAX;
    if (job == JOB_ADJ && sharded) return KCCOT_SMOOTH_CAUSAL_T | KCCOT_SMOOTH_STATS_ONLY | KCCOT_SMOOTH_EXTERNAL_STATS;
    return KCCOT_SMOOTH_CAUSAL_T;
}

int an_check_fwd_flags(const AnCall& c) {
    if ((c.flags & KCCOT_SMOOTH_NO_DIVIDE) && (c.flags & KCCOT_SMOOTH_EXTERNAL_MAX))
        return fail(KCCOT_EINVAL, "%s: KCCOT_SMOOTH_EXTERNAL_MAX and KCCOT_SMOOTH_NO_DIVIDE are exclusive", c.who);
    return 0;
}

// does the dsigma entry launch aniso_tile at all (else both results are exactly 0)
bool an_dsigma_launches(int rt, int rs) { return rt > 0 || rs > 0; }

TileSearch an_search_of(const AnCall& c, int job) { return an_search(c.B, c.H, c.T, c.W, c.C, c.rt, c.rs, c.causal(), job); }

// one walk: the geometry and the tables of the job, the grid checked against its area of the workspace
int an_walk(const AnCall& c, int job, AnArgs a, const AnAreas& w, int64_t* grid = nullptr) {
    const TileSearch q = an_search_of(c, job);
    const TilePlan pl = tile_plan(q);
    if (!pl.ok || (size_t)pl.grid * 2 * sizeof(double) > w.lay.part)        // (the layout was sized from this very plan)
        return fail(KCCOT_EUNSUPPORTED, "%s: no tiling for [%d,%d,%d,%d,%d] at radii (%d, %d)", c.who, c.B, c.H, c.T, c.W, c.C, c.rt, c.rs);
    if (grid) *grid = pl.grid;
    a.g = tile_geometry(q, pl);
    a.rt = c.rt;
    const SymD ss = make_sym_d(c.sigma_s, c.rs);
    for (int k = 0; k <= 2 * c.rs; ++k) { a.ws[k] = ss.w[k]; a.dws[k] = ss.dw[k]; }
    if (job == JOB_ADJ) {
        a.tab[1] = tab_reflect_adj(ss.w, c.rs, c.W);
        a.tab[2] = tab_reflect_adj(ss.w, c.rs, c.H);
    }
    if (c.causal()) {
        const CausD cd = make_caus_d(c.sigma_t, c.rt);
        a.kind_t = ROW_HEAD;
        if (job == JOB_ADJ) { a.tb = 0; a.ta = c.rt; a.halo_t = HALO_ZERO; a.tab[0] = tab_causal_adj(cd.v, c.rt); }
        else {
            a.tb = c.rt; a.ta = 0; a.halo_t = HALO_CLAMP; a.tab[0] = tab_causal_fwd(cd.v, c.rt);
            if (job == JOB_DSIG) a.tab[1] = tab_causal_fwd(cd.dv, c.rt);
        }
    } else {
        const SymD st = make_sym_d(c.sigma_t, c.rt);
        a.tb = a.ta = c.rt;
        if (job == JOB_ADJ) { a.kind_t = ROW_BORDER; a.halo_t = HALO_ZERO; a.tab[0] = tab_reflect_adj(st.w, c.rt, c.T); }
        else {
            a.kind_t = ROW_UNIFORM; a.halo_t = HALO_REFLECT; a.tab[0] = tab_uniform(st.w, c.rt);
            if (job == JOB_DSIG) a.tab[1] = tab_uniform(st.dw, c.rt);
        }
    }
    switch (c.rs) {
        case 0: return launch_tile_rs<0>(job, pl, a, c.st);
        case 1: return launch_tile_rs<1>(job, pl, a, c.st);
        case 2: return launch_tile_rs<2>(job, pl, a, c.st);
        case 3: return launch_tile_rs<3>(job, pl, a, c.st);
        case 4: return launch_tile_rs<4>(job, pl, a, c.st);
        case 5: return launch_tile_rs<5>(job, pl, a, c.st);
        case 6: return launch_tile_rs<6>(job, pl, a, c.st);
        default: return launch_tile_rs<7>(job, pl, a, c.st);
    }
}

int an_bwd(const AnCall& c, const float* gout, const float* out, const float* max_in, float* stats_ext, float* din) {
    const bool stats_only = (c.flags & KCCOT_SMOOTH_STATS_ONLY) != 0, stats_in = (c.flags & KCCOT_SMOOTH_EXTERNAL_STATS) != 0;
    int rc;
    if ((rc = an_check(c, an_allowed(JOB_ADJ, stats_ext != nullptr)))) return rc;
    if (!gout || !out || !max_in || (!stats_only && !din)) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    if ((rc = an_check_ws(c))) return rc;
    const AnAreas w(c);
    float* stats = (stats_only || stats_in) ? stats_ext : w.scal();
    if (!stats_in && (rc = an_stats(c, gout, out, w, stats))) return rc;
    if (stats_only) return 0;
    AnArgs a{};
    a.gout = gout; a.outf = out; a.mx = max_in; a.stats = stats; a.res = din;
    return an_walk(c, JOB_ADJ, a, w);
}

}  // namespace

}  // namespace kccot

using namespace kccot;

extern "C" int kccot_smooth_aniso_plan(int B, int H, int T, int W, int C, int radius_t, int radius_s, unsigned flags, int job, int* out) {
    // (the sigmas and the workspace play no part in the tiling: placeholders that pass their checks)
    const AnCall c{"smooth_aniso_plan", B, H, T, W, C, 1.f, 1.f, radius_t, radius_s, flags, nullptr, 0, nullptr};
    int rc;
    if (job != JOB_FWD && job != JOB_ADJ && job != JOB_DSIG) return fail(KCCOT_EINVAL, "%s: job %d is none of 0 (forward), 1 (adjoint), 2 (dsigma)", c.who, job);
    // the adjoint: the bits of either backward entry point
    if ((rc = an_check(c, an_allowed(job, job == JOB_ADJ)))) return rc;
    if (job == JOB_FWD && (rc = an_check_fwd_flags(c))) return rc;
    if (!out) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    if ((rc = an_check_size(c))) return rc;
    for (int k = 0; k < KCCOT_SMOOTH_ANISO_PLAN_INTS; ++k) out[k] = 0;
    if (job == JOB_DSIG && !an_dsigma_launches(radius_t, radius_s)) return 0;
    const TileSearch q = an_search_of(c, job);
    const TilePlan pl = tile_plan(q);
    if (!pl.ok) return fail(KCCOT_EUNSUPPORTED, "%s: no tiling for [%d,%d,%d,%d,%d] at radii (%d, %d)", c.who, B, H, T, W, C, radius_t, radius_s);
    const TileGeom g = tile_geometry(q, pl);
    const int v[KCCOT_SMOOTH_ANISO_PLAN_INTS] = {1, radius_s, pl.ni, job, g.tt, g.wt, g.ct, g.hs, g.ntt, g.ntw, g.ntc, g.nseg, (int)pl.grid};
    for (int k = 0; k < KCCOT_SMOOTH_ANISO_PLAN_INTS; ++k) out[k] = v[k];
    return 0;
}

extern "C" size_t kccot_smooth_aniso_workspace_bytes(int B, int H, int T, int W, int C) {
    if (B <= 0 || H <= 0 || T <= 0 || W <= 0 || C <= 0) return 0;
    return AnWs(B, H, T, W, C).total;
}

extern "C" int kccot_smooth_aniso_fwd_f32(const float* in, int B, int H, int T, int W, int C, float sigma_t, int radius_t,
                                          float sigma_s, int radius_s, unsigned flags, float* out, float* max_inout, void* ws,
                                          size_t ws_bytes, kccot_stream_t stream) {
    const AnCall c{"smooth_aniso_fwd", B, H, T, W, C, sigma_t, sigma_s, radius_t, radius_s, flags, ws, ws_bytes, (hipStream_t)stream};
    const bool nodiv = (flags & KCCOT_SMOOTH_NO_DIVIDE) != 0, ext = (flags & KCCOT_SMOOTH_EXTERNAL_MAX) != 0;
    int rc;
    if ((rc = an_check(c, an_allowed(JOB_FWD)))) return rc;
    if ((rc = an_check_fwd_flags(c))) return rc;
    if (!in || !out || !max_inout) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    if (in == out) return fail(KCCOT_EINVAL, "%s: in-place smoothing is not supported", c.who);
    if ((rc = an_check_ws(c))) return rc;
    const AnAreas w(c);
    AnArgs a{};
    a.in = in; a.res = out; a.bmax = w.bmax();
    int64_t grid = 0;
    if ((rc = an_walk(c, JOB_FWD, a, w, &grid))) return rc;
    if (!ext) {
        hipLaunchKernelGGL(aniso_reduce_max, dim3(1), dim3(1024), 0, c.st, (const float*)w.bmax(), grid, max_inout);
        if ((rc = launch_status("aniso_reduce_max"))) return rc;
    }
    if (nodiv) return 0;
    const int64_t nb = (c.n() + 255) / 256;
    hipLaunchKernelGGL(aniso_divide, dim3((unsigned)(nb < 65536 ? nb : 65536)), dim3(256), 0, c.st, out, c.n(), (const float*)max_inout);
    return launch_status("aniso_divide");
}

extern "C" int kccot_smooth_aniso_bwd_f32(const float* gout, const float* out, const float* max_in, int B, int H, int T, int W,
                                          int C, float sigma_t, int radius_t, float sigma_s, int radius_s, unsigned flags,
                                          float* din, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const AnCall c{"smooth_aniso_bwd", B, H, T, W, C, sigma_t, sigma_s, radius_t, radius_s, flags, ws, ws_bytes, (hipStream_t)stream};
    return an_bwd(c, gout, out, max_in, nullptr, din);
}

extern "C" int kccot_smooth_aniso_bwd_sharded_f32(const float* gout, const float* out, const float* max_in, float* stats_inout,
                                                  int B, int H, int T, int W, int C, float sigma_t, int radius_t, float sigma_s,
                                                  int radius_s, unsigned flags, float* din, void* ws, size_t ws_bytes,
                                                  kccot_stream_t stream) {
    const AnCall c{"smooth_aniso_bwd_sharded", B, H, T, W, C, sigma_t, sigma_s, radius_t, radius_s, flags, ws, ws_bytes, (hipStream_t)stream};
    const unsigned both = KCCOT_SMOOTH_STATS_ONLY | KCCOT_SMOOTH_EXTERNAL_STATS;
    const int rc = an_check_flags(c, an_allowed(JOB_ADJ, true));
    if (rc) return rc;
    if (!(flags & both) || (flags & both) == both)
        return fail(KCCOT_EINVAL, "%s: exactly one of KCCOT_SMOOTH_STATS_ONLY and KCCOT_SMOOTH_EXTERNAL_STATS", c.who);
    if (!stats_inout) return fail(KCCOT_EINVAL, "%s: null stats pointer", c.who);
    return an_bwd(c, gout, out, max_in, stats_inout, din);
}

extern "C" int kccot_smooth_aniso_dsigma_f32(const float* in, const float* gout, const float* out, const float* max_in,
                                             const float* stats_in, int B, int H, int T, int W, int C, float sigma_t,
                                             int radius_t, float sigma_s, int radius_s, unsigned flags, float* dsigma_out,
                                             void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const AnCall c{"smooth_aniso_dsigma", B, H, T, W, C, sigma_t, sigma_s, radius_t, radius_s, flags, ws, ws_bytes, (hipStream_t)stream};
    int rc;
    if ((rc = an_check(c, an_allowed(JOB_DSIG)))) return rc;
    if (!in || !gout || !out || !max_in || !dsigma_out) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    if ((rc = an_check_ws(c))) return rc;
    const AnAreas w(c);
    int64_t nparts = 0;
    if (an_dsigma_launches(radius_t, radius_s)) {
        const float* stats = stats_in;
        if (!stats) {
            if ((rc = an_stats(c, gout, out, w, w.scal()))) return rc;
            stats = w.scal();
        }
        AnArgs a{};
        a.in = in; a.gout = gout; a.outf = out; a.mx = max_in; a.stats = stats; a.part = w.part();
        if ((rc = an_walk(c, JOB_DSIG, a, w, &nparts))) return rc;
    }
    // (a component whose axis group has radius 0 is written as 0)
    hipLaunchKernelGGL(tile_combine<2>, dim3(1), dim3(1024), 0, c.st, (const double*)w.part(), nparts,
                       (radius_t > 0 ? 1u : 0u) | (radius_s > 0 ? 2u : 0u), dsigma_out);
    return launch_status("tile_combine");
}
