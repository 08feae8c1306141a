// Per-frame SSIM, its adjoint with respect to y, and the mean squared error behind PSNR (include/kccot_metrics.h; NOT reference
// behaviour: the reference publishes no sample-quality figure).  The definition is in the header.
//
// ssim_walk: ONE walk along H serves both jobs.  A workgroup owns, of one frame (b,t), a tile of wt columns and ct channels and a
// segment of hs rows.  A thread owns one column and channel of the tile.  Per image row: the row segments of x and y with their
// column halo go global -> LDS once (through a table of offsets within a row, built once; rows are contiguous in W*C, so with
// ct == C the loads are contiguous) -> W stencil on the five moment images x, y, x^2, y^2, xy (the products are formed from the
// LDS values on the fly, the stencil strides by ct) -> five (2R + 1)-deep REGISTER windows -> H stencil -> the job's epilogue.
//   forward   the tile is a tile of MAP columns; the epilogue evaluates S and adds it up in fp64.  The load stage also adds up
//             (x - y)^2 in fp64 over the elements the workgroup OWNS (its own columns and rows; the last tile and the last segment
//             also own their halo, which no other workgroup's own part covers): every element of the frame is counted once.  Two
//             fp64 partials per workgroup; ssim_combine (one thread per frame) adds a frame's partials in workgroup order.
//   backward  FUSED: the tile is a tile of dy columns.  The moments run on the map columns that reach into the tile (the tile and
//             2R columns in front of it, as far as they lie inside the map: a tile of the whole width needs W - 2R threads per
//             channel for them and W for dy), on input rows 2R further back: the epilogue forms the three coefficient maps
//             u gamma, u alpha, u beta (zero outside the map), puts their row in LDS, the threads of the tile gather it along W
//             (G^T) into three more register windows, gather along H and write dy = G^T(u gamma) + 2 y G^T(u alpha) +
//             x G^T(u beta) with the x and y of that element read again (a row that went through the walk 2R steps earlier).
//             No coefficient map touches HBM and the workspace is not used.
// R, the radius, is a template argument because of the windows.  No float atomics: the same call gives the same bits.
#include "common.h"
#include "smooth_internal.h"
#include "../../include/kccot_metrics.h"
#include <math.h>
#include <stdint.h>

namespace kccot {

namespace {

constexpr int SS_NT = 256;                          // most threads of a workgroup = most (column, channel) positions of a tile
constexpr int SS_CT = 16;                           // most channels of a tile
constexpr int SS_NIN = SS_NT + 2 * SM_MAXR * SS_CT; // most floats of an LDS input row: the positions and 2R more columns
constexpr int64_t SS_FILL = 1024;                   // workgroups the chip should see before segments stop being cut

struct SsArgs {
    const float* x;
    const float* y;
    const float* g;         // backward: [B*T]
    float* dy;              // backward
    double* part;           // forward: two partials per workgroup
    int H, T, W, C;
    int wt, ct, hs;         // tile extents along W and C, the segment along H
    int ntw, ntc, nseg;
    float c1, c2;
    float cnt;              // backward: (H - 2R)(W - 2R) C
    float w[2 * SM_MAXR + 1];
};

template <int R, bool BWD>
__global__ __launch_bounds__(SS_NT) void ssim_walk(SsArgs a) {
    constexpr int NW = 2 * R + 1;
    __shared__ float X[SS_NIN], Y[SS_NIN];
    __shared__ int xoff[SS_NIN];                    // offset within an image row; ~offset: not owned (forward), or outside
    __shared__ float M[3][BWD ? SS_NIN : 1];        // backward: one row of u gamma, u alpha, u beta at map columns q0 - 2R ..
    __shared__ double wpart[2][SS_NT / 64];
    const int tid = threadIdx.x, nt = blockDim.x;
    int blk = blockIdx.x;
    const int tc = blk % a.ntc; blk /= a.ntc;
    const int tw = blk % a.ntw; blk /= a.ntw;
    const int seg = blk % a.nseg, f = blk / a.nseg;
    const int b = f / a.T, t = f - b * a.T;
    const int Hm = a.H - 2 * R, Wm = a.W - 2 * R;
    const int ct = a.ct, c0 = tc * ct, q0 = tw * a.wt;      // q0: the first map column (forward) / dy column (backward)
    const int xcol0 = BWD ? max(q0 - 2 * R, 0) : q0;        // the image column of LDS column 0 = the map column of position 0
    const int ncol = BWD ? min(q0 + a.wt, Wm) - xcol0 : a.wt;   // position columns of the moments (backward: inside the map)
    const int mshift = BWD ? (xcol0 - (q0 - 2 * R)) * ct : 0;   // backward: position 0 within a row of M
    const int nin = (ncol + 2 * R) * ct;
    const int r0 = seg * a.hs, r1 = min(r0 + a.hs, BWD ? a.H : Hm);    // owned rows: of the map (forward) / of dy (backward)
    const int start = BWD ? max(r0 - 2 * R, 0) : r0, end = r1 + 2 * R; // image rows of the walk
    const bool last_w = tw == a.ntw - 1, last_h = seg == a.nseg - 1;

    for (int e = tid; e < nin; e += nt) {
        const int wc = e / ct, cc = e - wc * ct;
        const int wraw = xcol0 + wc, craw = c0 + cc;
        const bool inside = wraw >= 0 && wraw < a.W && craw < a.C;
        const int wg = wraw < 0 ? 0 : (wraw > a.W - 1 ? a.W - 1 : wraw);    // (clamped: only a masked position reads it)
        const int off = wg * a.C + min(craw, a.C - 1);
        const bool own = !BWD && inside && (wc < a.wt || last_w);
        xoff[e] = own ? off : ~off;
    }
    // this thread's position: column ml and channel cl of the tile; its first tap sits at X[tid]
    const int ml = tid / ct, cl = tid - ml * ct;
    const bool pos = tid < ncol * ct;
    const int jcol = xcol0 + ml;
    const bool valid_m = pos && jcol < Wm && c0 + cl < a.C;
    const bool gat = BWD && tid < a.wt * ct;                // backward: a position of the dy tile
    const bool valid_d = gat && q0 + ml < a.W && c0 + cl < a.C;
    const int64_t rowpitch = (int64_t)a.T * a.W * a.C;
    const int64_t fbase = ((int64_t)b * a.H * a.T + t) * ((int64_t)a.W * a.C);
    const int doff = valid_d ? (q0 + ml) * a.C + c0 + cl : 0;
    const float u = BWD ? a.g[f] / a.cnt : 0.f;

    float wx[NW], wy[NW], wxx[NW], wyy[NW], wxy[NW];
    float mg[BWD ? NW : 1], ma[BWD ? NW : 1], mb[BWD ? NW : 1];
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        wx[j] = 0.f; wy[j] = 0.f; wxx[j] = 0.f; wyy[j] = 0.f; wxy[j] = 0.f;
        if (BWD) { mg[j] = 0.f; ma[j] = 0.f; mb[j] = 0.f; }
    }
    if (BWD)                                    // the columns of M outside the map stay zero: no position writes them
        for (int e = tid; e < (a.wt + 2 * R) * ct; e += nt) { M[0][e] = 0.f; M[1][e] = 0.f; M[2][e] = 0.f; }
    double acc_s = 0.0, acc_m = 0.0;
    for (int hp = start; hp < end; ++hp) {
        const bool have = hp < a.H;                 // (backward: the last 2R steps only drain the windows; uniform)
        float fx = 0.f, fy = 0.f, fxx = 0.f, fyy = 0.f, fxy = 0.f;
        if (have) {
            const float* xp = a.x + fbase + (int64_t)hp * rowpitch;
            const float* yp = a.y + fbase + (int64_t)hp * rowpitch;
            const bool own_row = !BWD && (hp < r1 || last_h);
            __syncthreads();                        // the table (first step); the W stage of the step before has read X, Y
            for (int e = tid; e < nin; e += nt) {
                int o = xoff[e];
                const bool own = o >= 0;
                o = own ? o : ~o;
                const float xv = xp[o], yv = yp[o];
                X[e] = xv; Y[e] = yv;
                if (!BWD && own && own_row) {
                    const double d = (double)(xv - yv);
                    acc_m = fma(d, d, acc_m);
                }
            }
            __syncthreads();
            if (pos) {
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    const float xv = X[tid + k * ct], yv = Y[tid + k * ct], wk = a.w[k];
                    fx = fmaf(wk, xv, fx); fy = fmaf(wk, yv, fy);
                    fxx = fmaf(wk, xv * xv, fxx); fyy = fmaf(wk, yv * yv, fyy); fxy = fmaf(wk, xv * yv, fxy);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < NW - 1; ++j) { wx[j] = wx[j + 1]; wy[j] = wy[j + 1]; wxx[j] = wxx[j + 1]; wyy[j] = wyy[j + 1]; wxy[j] = wxy[j + 1]; }
        wx[NW - 1] = fx; wy[NW - 1] = fy; wxx[NW - 1] = fxx; wyy[NW - 1] = fyy; wxy[NW - 1] = fxy;
        const int i = hp - 2 * R;                   // the map row this step completes
        const bool full = have && i >= start;       // (uniform)
        float cg = 0.f, ca = 0.f, cb = 0.f;
        if (full && valid_m) {
            float mx = 0.f, my = 0.f, gxx = 0.f, gyy = 0.f, gxy = 0.f;
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                const float wj = a.w[j];
                mx = fmaf(wj, wx[j], mx); my = fmaf(wj, wy[j], my);
                gxx = fmaf(wj, wxx[j], gxx); gyy = fmaf(wj, wyy[j], gyy); gxy = fmaf(wj, wxy[j], gxy);
            }
            // R == 0: one tap of weight 1, so G(x^2) = fl(x x) and the three differences are 0 in a plain fp32 evaluation; written
            // out as differences, the compiler's fma contraction would leave the rounding error of each product there instead
            const float sxx = R == 0 ? 0.f : gxx - mx * mx, syy = R == 0 ? 0.f : gyy - my * my, sxy = R == 0 ? 0.f : gxy - mx * my;
            const float A1 = 2.f * mx * my + a.c1, A2 = 2.f * sxy + a.c2;
            const float B1 = mx * mx + my * my + a.c1, B2 = sxx + syy + a.c2;
            const float S = (A1 * A2) / (B1 * B2);
            if (!BWD) acc_s += (double)S;
            else {
                const float alpha = -S / B2, beta = 2.f * A1 / (B1 * B2);
                const float gamma = 2.f * mx * A2 / (B1 * B2) - 2.f * my * S / B1 - beta * mx - 2.f * alpha * my;
                cg = u * gamma; ca = u * alpha; cb = u * beta;
            }
        }
        if (BWD) {
            if (!have) __syncthreads();             // (else the two barriers above lie behind the last reads of M)
            if (pos) { M[0][mshift + tid] = cg; M[1][mshift + tid] = ca; M[2][mshift + tid] = cb; }
            __syncthreads();
            float hg = 0.f, ha = 0.f, hb = 0.f;
            if (gat) {
                // (G^T m)[., q] = sum_b w_b m[., q - b]: dy column q0 + ml, map column q0 + ml - b = position ml + 2R - b
#pragma unroll
                for (int k = 0; k < NW; ++k) {
                    const float wk = a.w[k];
                    const int p = tid + (2 * R - k) * ct;
                    hg = fmaf(wk, M[0][p], hg); ha = fmaf(wk, M[1][p], ha); hb = fmaf(wk, M[2][p], hb);
                }
            }
#pragma unroll
            for (int j = 0; j < NW - 1; ++j) { mg[j] = mg[j + 1]; ma[j] = ma[j + 1]; mb[j] = mb[j + 1]; }
            mg[NW - 1] = hg; ma[NW - 1] = ha; mb[NW - 1] = hb;
            // dy row i: map rows i - 2R .. i are the window's rows 0 .. 2R, the tap of row i - a' is w[a']
            if (i >= r0 && valid_d) {
                float dg = 0.f, da = 0.f, db = 0.f;
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    const float wj = a.w[2 * R - j];
                    dg = fmaf(wj, mg[j], dg); da = fmaf(wj, ma[j], da); db = fmaf(wj, mb[j], db);
                }
                const int64_t o = fbase + (int64_t)i * rowpitch + doff;
                a.dy[o] = dg + 2.f * a.y[o] * da + a.x[o] * db;
            }
        }
    }
    if (!BWD) {
        acc_s = wave_sum_d(acc_s);
        acc_m = wave_sum_d(acc_m);
        if ((tid & 63) == 0) { wpart[0][tid >> 6] = acc_s; wpart[1][tid >> 6] = acc_m; }
        __syncthreads();
        if (tid < 2) {
            double s = 0.0;
            for (int w = 0; w < (nt >> 6); ++w) s += wpart[tid][w];
            a.part[2 * (int64_t)blockIdx.x + tid] = s;
        }
    }
}

// one thread per frame adds the frame's `per` partials in workgroup order
__global__ __launch_bounds__(256) void ssim_combine(const double* __restrict__ part, int per, int frames, double cnt_s, double cnt_m,
                                                    float* __restrict__ ssim_out, float* __restrict__ mse_out) {
    const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= frames) return;
    double s = 0.0, m = 0.0;
    for (int k = 0; k < per; ++k) { s += part[2 * (f * per + k)]; m += part[2 * (f * per + k) + 1]; }
    ssim_out[f] = (float)(s / cnt_s);
    if (mse_out) mse_out[f] = (float)(m / cnt_m);
}

// ---- the tiling ----------------------------------------------------------------------------------------------------------------
struct SsPlan { int wt, ct, hs, nt, ntw, ntc, nseg; int64_t tiles, grid; };

// Forward: wt ct <= 256 positions of the map.  Backward: the dy tile and the map columns that reach into it, min(wt + 2r, W - 2r)
// of them, each within 256 positions: the whole width where W ct <= 256, else (wt + 2r) ct <= 256.
// ct = C up to 16 channels (a row segment is then contiguous); a smaller power of two where that buys a wider tile than the
// strided loads cost.  Segments along H are cut while the chip sees fewer than SS_FILL workgroups, never shorter than the rows a
// segment walks through on top of its own (2r forward, 4r backward).
SsPlan ss_plan(int B, int H, int T, int W, int C, int r, bool bwd) {
    const int halo = bwd ? 2 * r : 0, Wown = bwd ? W : W - 2 * r, Hown = bwd ? H : H - 2 * r;
    SsPlan best{};
    double best_cost = 1e300;
    const int ct0 = C < SS_CT ? C : SS_CT;
    for (int ct = ct0; ct >= 1;) {
        int wt = SS_NT / ct - halo;
        if (wt > Wown || (bwd && (int64_t)W * ct <= SS_NT)) wt = Wown;
        if (wt >= 1) {
            const double cost = (double)(wt + halo + 2 * r) / wt * (ct < C ? (double)SS_CT / ct : 1.0);
            if (cost < best_cost) {
                best_cost = cost;
                best.wt = wt; best.ct = ct;
            }
        }
        if (ct == 1) break;
        int p = 1;
        while (p * 2 < ct) p *= 2;                  // the next power of two below ct
        ct = p;
    }
    // threads: the positions of the moments, and of dy
    const int nmc = bwd ? (best.wt + halo < W - 2 * r ? best.wt + halo : W - 2 * r) : best.wt;
    best.nt = ((nmc > best.wt ? nmc : best.wt) * best.ct + 63) / 64 * 64;
    best.ntw = (int)(((int64_t)Wown + best.wt - 1) / best.wt);
    best.ntc = (int)(((int64_t)C + best.ct - 1) / best.ct);
    best.tiles = (int64_t)best.ntw * best.ntc;
    const double n = (double)B * T * (double)best.tiles;
    const int min_hs = (bwd ? 4 : 2) * r > 4 ? (bwd ? 4 : 2) * r : 4;
    int64_t nseg = n >= (double)SS_FILL ? 1 : (int64_t)(((double)SS_FILL + n - 1) / n);
    if (nseg > Hown / min_hs) nseg = Hown / min_hs;
    if (nseg < 1) nseg = 1;
    best.hs = (int)((Hown + nseg - 1) / nseg);
    best.nseg = (Hown + best.hs - 1) / best.hs;
    best.grid = n * best.nseg > 4e18 ? INT64_MAX : (int64_t)B * T * best.tiles * best.nseg;
    return best;
}

struct SsCall {
    const char* who;
    int B, H, T, W, C;
    float sigma;
    int r;
    float L;
    void* ws;
    size_t ws_bytes;
    hipStream_t st;
};

// Workspace: [two doubles per workgroup of the forward].  nseg <= ceil(SS_FILL / n) with n = B T tiles, so a grid is below
// n + SS_FILL: the area is sized for that at the radius with the most tiles (a bound that grows with B; the launch checks its
// grid against it again).  + 256: the area starts at the next 256-byte boundary of ws.
size_t ss_ws_bytes(int B, int H, int T, int W, int C) {
    double nmax = 0.0;
    for (int r = 0; r <= SM_MAXR && 2 * r < H && 2 * r < W; ++r) {
        const double n = (double)B * T * (double)ss_plan(B, H, T, W, C, r, false).tiles;
        if (n > nmax) nmax = n;
    }
    if (nmax > 1e15) return ~(size_t)0 - 255;       // (a tensor too large to index: refused before the workspace is looked at)
    return up256(((size_t)nmax + (size_t)SS_FILL) * 2 * sizeof(double)) + 256;
}

int ss_check(const SsCall& c) {
    if (c.B <= 0 || c.H <= 0 || c.T <= 0 || c.W <= 0 || c.C <= 0)
        return fail(KCCOT_EINVAL, "%s: bad shape [%d,%d,%d,%d,%d]", c.who, c.B, c.H, c.T, c.W, c.C);
    if (!(c.sigma > 0.f)) return fail(KCCOT_EINVAL, "%s: sigma must be > 0", c.who);
    if (!(c.L > 0.f)) return fail(KCCOT_EINVAL, "%s: data_range must be > 0", c.who);
    if (c.r < 0 || c.r > SM_MAXR) return fail(KCCOT_EINVAL, "%s: radius %d outside 0..%d", c.who, c.r, SM_MAXR);
    if (2 * c.r >= c.H || 2 * c.r >= c.W)
        return fail(KCCOT_EINVAL, "%s: the window of %d does not fit a %d x %d frame", c.who, 2 * c.r + 1, c.H, c.W);
    return 0;
}

// too large to index: the entry points and kccot_ssim_plan
int ss_check_index(const SsCall& c, const SsPlan& pl) {
    if ((int64_t)c.B * c.T > 0x7fffffff || (int64_t)c.W * c.C > 0x7fffffff || pl.tiles > 0x7fffffff || pl.grid > 0x7fffffff ||
        (double)c.B * c.H * c.T * (double)c.W * c.C > 4e18)
        return fail(KCCOT_EUNSUPPORTED, "%s: tensor [%d,%d,%d,%d,%d] too large to index", c.who, c.B, c.H, c.T, c.W, c.C);
    return 0;
}

// after the argument checks: too large to index, then the workspace
int ss_check_size(const SsCall& c, const SsPlan& pl) {
    const int rc = ss_check_index(c, pl);
    if (rc) return rc;
    const size_t need = ss_ws_bytes(c.B, c.H, c.T, c.W, c.C);
    if (!c.ws || c.ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", c.who, c.ws_bytes, need);
    return 0;
}

template <int R>
int ss_launch_r(bool bwd, const SsPlan& pl, const SsArgs& a, hipStream_t st) {
    if (bwd) hipLaunchKernelGGL((ssim_walk<R, true>), dim3((unsigned)pl.grid), dim3(pl.nt), 0, st, a);
    else hipLaunchKernelGGL((ssim_walk<R, false>), dim3((unsigned)pl.grid), dim3(pl.nt), 0, st, a);
    return launch_status("ssim_walk");
}

int ss_launch(const SsCall& c, bool bwd, const SsPlan& pl, SsArgs a) {
    a.H = c.H; a.T = c.T; a.W = c.W; a.C = c.C;
    a.wt = pl.wt; a.ct = pl.ct; a.hs = pl.hs; a.ntw = pl.ntw; a.ntc = pl.ntc; a.nseg = pl.nseg;
    a.c1 = (float)((0.01 * (double)c.L) * (0.01 * (double)c.L));
    a.c2 = (float)((0.03 * (double)c.L) * (0.03 * (double)c.L));
    a.cnt = (float)((double)(c.H - 2 * c.r) * (c.W - 2 * c.r) * c.C);
    const Taps tp = make_taps(c.sigma, c.r);
    for (int k = 0; k <= 2 * c.r; ++k) a.w[k] = tp.w[k];
    switch (c.r) {
        case 0: return ss_launch_r<0>(bwd, pl, a, c.st);
        case 1: return ss_launch_r<1>(bwd, pl, a, c.st);
        case 2: return ss_launch_r<2>(bwd, pl, a, c.st);
        case 3: return ss_launch_r<3>(bwd, pl, a, c.st);
        case 4: return ss_launch_r<4>(bwd, pl, a, c.st);
        case 5: return ss_launch_r<5>(bwd, pl, a, c.st);
        case 6: return ss_launch_r<6>(bwd, pl, a, c.st);
        default: return ss_launch_r<7>(bwd, pl, a, c.st);
    }
}

bool ss_overlap(const float* p, const float* q, double n) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    const double bytes = 4.0 * n;
    return a == b || (a < b ? (double)(b - a) < bytes : (double)(a - b) < bytes);
}

}  // namespace

}  // namespace kccot

using namespace kccot;

extern "C" int kccot_ssim_plan(int B, int H, int T, int W, int C, int radius, int backward, int* out) {
    // (sigma, data_range and the workspace play no part in the tiling: placeholders that pass their checks)
    const SsCall c{"ssim_plan", B, H, T, W, C, 1.f, radius, 1.f, nullptr, 0, nullptr};
    int rc;
    if ((rc = ss_check(c))) return rc;
    if (!out) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    const SsPlan pl = ss_plan(B, H, T, W, C, radius, backward != 0);
    if ((rc = ss_check_index(c, pl))) return rc;
    const int v[KCCOT_SSIM_PLAN_INTS] = {pl.wt, pl.ct, pl.hs, pl.nt, pl.ntw, pl.ntc, pl.nseg, (int)pl.grid};
    for (int k = 0; k < KCCOT_SSIM_PLAN_INTS; ++k) out[k] = v[k];
    return 0;
}

extern "C" size_t kccot_ssim_workspace_bytes(int B, int H, int T, int W, int C) {
    if (B <= 0 || H <= 0 || T <= 0 || W <= 0 || C <= 0) return 0;
    return ss_ws_bytes(B, H, T, W, C);
}

extern "C" int kccot_ssim_fwd_f32(const float* x, const float* y, int B, int H, int T, int W, int C, float sigma, int radius,
                                  float data_range, float* ssim_out, float* mse_out, void* ws, size_t ws_bytes,
                                  kccot_stream_t stream) {
    const SsCall c{"ssim_fwd", B, H, T, W, C, sigma, radius, data_range, ws, ws_bytes, (hipStream_t)stream};
    int rc;
    if ((rc = ss_check(c))) return rc;
    if (!x || !y || !ssim_out) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    const SsPlan pl = ss_plan(B, H, T, W, C, radius, false);
    if ((rc = ss_check_size(c, pl))) return rc;
    double* part = reinterpret_cast<double*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    if ((size_t)pl.grid * 2 * sizeof(double) + 256 > ws_bytes)      // (the workspace was sized from a bound on this very grid)
        return fail(KCCOT_EWORKSPACE, "%s: workspace %zu too small for %lld workgroups", c.who, ws_bytes, (long long)pl.grid);
    SsArgs a{};
    a.x = x; a.y = y; a.part = part;
    if ((rc = ss_launch(c, false, pl, a))) return rc;
    const int frames = B * T, per = (int)(pl.tiles * pl.nseg);
    hipLaunchKernelGGL(ssim_combine, dim3((unsigned)(((int64_t)frames + 255) / 256)), dim3(256), 0, c.st, (const double*)part, per, frames,
                       (double)(H - 2 * radius) * (W - 2 * radius) * C, (double)H * W * C, ssim_out, mse_out);
    return launch_status("ssim_combine");
}

extern "C" int kccot_ssim_bwd_f32(const float* g, const float* x, const float* y, int B, int H, int T, int W, int C, float sigma,
                                  int radius, float data_range, float* dy, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const SsCall c{"ssim_bwd", B, H, T, W, C, sigma, radius, data_range, ws, ws_bytes, (hipStream_t)stream};
    int rc;
    if ((rc = ss_check(c))) return rc;
    if (!g || !x || !y || !dy) return fail(KCCOT_EINVAL, "%s: null pointer", c.who);
    const double n = (double)B * H * T * (double)W * C;
    if (ss_overlap(dy, x, n) || ss_overlap(dy, y, n)) return fail(KCCOT_EINVAL, "%s: dy must not alias x or y", c.who);
    const SsPlan pl = ss_plan(B, H, T, W, C, radius, true);
    if ((rc = ss_check_size(c, pl))) return rc;
    SsArgs a{};
    a.x = x; a.y = y; a.g = g; a.dy = dy;
    return ss_launch(c, true, pl, a);
}
