// Adjoint of the L1 ground cost C[i,j] = sc * sum_k |x[i,k] - y[j,k]| (include/kccot_l1.h; NOT reference behaviour: the forward is
// the flag KCCOT_COST_L1 of the direct-difference kernel in cost.hip).
//
// sgn(y[j,k] - x[i,k]) depends on (i, j, k) together, so the gradient is no GEMM and never reaches the matrix pipe.  Every form
// of the header (dx, dy, x == y, the loss's dfake) is
//     out[r,k] = sc * sum_{c<N} W[r,c] * sgn(a[r,k] - S[c,k])
// with a the target rows, S the source rows (one or two row blocks, read in place) and W [R,N] a coefficient matrix made of g.
//
//   l1_build_coeffs : W transposed, Wt[c][r], rows padded to a multiple of L1_RR with zeros -- the only thing in the workspace.
//   l1_sign_apply   : a workgroup owns L1_RR target rows x 1024 columns; a lane owns 4 columns (one float4 where rows are 16-byte
//                     aligned, else 4 columns 256 apart, so that either way a wave's loads are coalesced) and keeps the L1_RR x 4
//                     values of `a` and as many accumulators in registers.  The source rows stream past straight from global
//                     memory, L1_UN rows in flight; Wt[c][r0..r0+8) is wave-uniform (scalar loads, one 32-byte line per source
//                     row).  Each loaded source value feeds L1_RR sign-FMAs; the sources are read ceil(R / L1_RR) times in all.
//
// The sign is two fp32 comparisons of the two values and two selects (+1, -1 or 0), then one FMA with the coefficient: 5 VALU
// issues per pair.  Comparing a with s is comparing a - s with 0 (fp32 subtraction with gradual underflow never rounds a
// non-zero difference to 0), and a tie gives a multiplier of exactly 0: it adds +0 * W, whatever W is.  copysign alone would
// turn a tie into +-W.  The sum over c runs c = 0..N-1 per element: a fixed order, no atomics.
#include "common.h"
#include "../../include/kccot_l1.h"

namespace kccot {

constexpr int L1_RR = 8;                    // target rows of a workgroup
constexpr int L1_KPL = 4;                   // columns of a lane
constexpr int L1_NT = 256;                  // threads of a workgroup
constexpr int L1_KT = L1_NT * L1_KPL;       // columns of a workgroup
constexpr int L1_UN = 4;                    // source rows in flight

enum L1Coef { L1_DX = 0, L1_DY = 1, L1_SAME = 2, L1_LOSS = 3 };

static inline int l1_pad(int R) { return (R + L1_RR - 1) / L1_RR * L1_RR; }

// Wt [N][Rp]: Wt[c * Rp + r] = W[r,c] for r < R, 0 for the padding rows.  g is [Bx,By] (g3 [3,B,B] with Bx = By = B for L1_LOSS).
__global__ __launch_bounds__(256) void l1_build_coeffs(int mode, const float* __restrict__ g, int Bx, int By, int R, int Rp,
                                                       int N, float* __restrict__ Wt) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)N * Rp) return;
    const int c = (int)(e / Rp), r = (int)(e % Rp);
    float w = 0.f;
    if (r < R) {
        if (mode == L1_DX) {                    // r = i, c = j
            w = g[(int64_t)r * By + c];
        } else if (mode == L1_DY) {             // r = j, c = i
            w = g[(int64_t)c * By + r];
        } else if (mode == L1_SAME) {
            w = g[(int64_t)r * By + c] + g[(int64_t)c * By + r];
        } else {                                // sources [real; fake]: gxy[i,j], then gyy[i,j] + gyy[j,i]; r = j
            const float* gyy = g + 2 * (int64_t)Bx * Bx;
            const int i = c < Bx ? c : c - Bx;
            w = c < Bx ? g[(int64_t)i * Bx + r] : gyy[(int64_t)i * Bx + r] + gyy[(int64_t)r * Bx + i];
        }
    }
    Wt[e] = w;
}

template <bool VEC>
__device__ __forceinline__ void l1_load(const float* __restrict__ row, const int64_t (&col)[L1_KPL], float (&v)[L1_KPL]) {
    if (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(row + col[0]);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int e = 0; e < L1_KPL; ++e) v[e] = row[col[e]];
    }
}

// acc[q][e] += w[q] * sgn(av[q][e] - sv[e]) for the L1_RR target rows of the workgroup
__device__ __forceinline__ void l1_step(const float (&av)[L1_RR][L1_KPL], const float (&sv)[L1_KPL], const float* __restrict__ w,
                                        float (&acc)[L1_RR][L1_KPL]) {
#pragma unroll
    for (int q = 0; q < L1_RR; ++q) {
        const float wq = w[q];
#pragma unroll
        for (int e = 0; e < L1_KPL; ++e) {
            const float up = av[q][e] > sv[e] ? 1.f : 0.f;
            const float sg = av[q][e] < sv[e] ? -1.f : up;      // a tie (and a NaN): 0
            acc[q][e] = fmaf(wq, sg, acc[q][e]);
        }
    }
}

// n source rows S [n,K] with their coefficients w = Wt + c_first * Rp + r0, in row order
template <bool VEC>
__device__ __forceinline__ void l1_walk(const float* __restrict__ S, int n, const float* __restrict__ w, int Rp, int64_t K,
                                        const int64_t (&col)[L1_KPL], const float (&av)[L1_RR][L1_KPL],
                                        float (&acc)[L1_RR][L1_KPL]) {
    if (n <= 0) return;
    // batches of L1_UN rows, the next batch's loads in flight while this one is consumed; rows past n - 1 are clamped to it
    // for the loads (no tail loop, no load behind a branch) and skipped by a wave-uniform test
    float cur[L1_UN][L1_KPL], nxt[L1_UN][L1_KPL];
#pragma unroll
    for (int u = 0; u < L1_UN; ++u) l1_load<VEC>(S + (int64_t)(u < n ? u : n - 1) * K, col, cur[u]);
    for (int c = 0; c < n; c += L1_UN) {
#pragma unroll
        for (int u = 0; u < L1_UN; ++u) {
            const int cn = c + L1_UN + u;
            l1_load<VEC>(S + (int64_t)(cn < n ? cn : n - 1) * K, col, nxt[u]);
        }
        float wc[L1_UN][L1_RR];
#pragma unroll
        for (int u = 0; u < L1_UN; ++u) {
            const float* wr = w + (int64_t)(c + u < n ? c + u : n - 1) * Rp;
#pragma unroll
            for (int q = 0; q < L1_RR; ++q) wc[u][q] = wr[q];
        }
        __builtin_amdgcn_sched_barrier(0);      // the loads above stay above: hipcc otherwise sinks each to its first use
#pragma unroll
        for (int u = 0; u < L1_UN; ++u)
            if (c + u < n) l1_step(av, cur[u], wc[u], acc);
#pragma unroll
        for (int u = 0; u < L1_UN; ++u)
#pragma unroll
            for (int e = 0; e < L1_KPL; ++e) cur[u][e] = nxt[u][e];
    }
}

// grid = (column tiles, row groups).  VEC: K % 4 == 0 and a, S1, S2, out 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(L1_NT) void l1_sign_apply(const float* __restrict__ a, const float* __restrict__ S1, int n1,
                                                       const float* __restrict__ S2, int n2, const float* __restrict__ Wt,
                                                       int R, int Rp, int64_t K, float sc, float* __restrict__ out) {
    const int t = threadIdx.x;
    const int64_t k0 = (int64_t)blockIdx.x * L1_KT;
    const int r0 = blockIdx.y * L1_RR;
    // columns past K are clamped to column 0 for the loads (no load depends on a branch) and never stored
    int64_t col[L1_KPL];
    bool ok[L1_KPL];
#pragma unroll
    for (int e = 0; e < L1_KPL; ++e) {
        const int64_t k = VEC ? k0 + 4 * t + e : k0 + t + (int64_t)L1_NT * e;
        ok[e] = k < K;
        col[e] = ok[e] ? k : (VEC ? e : 0);     // VEC: K % 4 == 0, so a lane's four columns are inside together or not at all
    }
    float av[L1_RR][L1_KPL], acc[L1_RR][L1_KPL];
#pragma unroll
    for (int q = 0; q < L1_RR; ++q) {
        const int r = r0 + q < R ? r0 + q : R - 1;              // rows past R: a valid row, coefficients 0, never stored
        l1_load<VEC>(a + (int64_t)r * K, col, av[q]);
#pragma unroll
        for (int e = 0; e < L1_KPL; ++e) acc[q][e] = 0.f;
    }
    const float* w = Wt + r0;
    l1_walk<VEC>(S1, n1, w, Rp, K, col, av, acc);
    l1_walk<VEC>(S2, n2, w + (int64_t)n1 * Rp, Rp, K, col, av, acc);
#pragma unroll
    for (int q = 0; q < L1_RR; ++q) {
        if (r0 + q >= R) break;
        float* o = out + (int64_t)(r0 + q) * K;
        if (VEC) {
            if (ok[0]) *reinterpret_cast<float4*>(o + col[0]) = make_float4(acc[q][0] * sc, acc[q][1] * sc, acc[q][2] * sc, acc[q][3] * sc);
        } else {
#pragma unroll
            for (int e = 0; e < L1_KPL; ++e)
                if (ok[e]) o[col[e]] = acc[q][e] * sc;
        }
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
static size_t l1_coef_bytes(int R, int N) { return up256((size_t)N * l1_pad(R) * sizeof(float)); }

static bool l1_overlap(const void* p, size_t pb, const void* q, size_t qb) {
    const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
    return p && q && a < b + qb && b < a + pb;
}

// what cannot be indexed: the row groups ride the y grid axis (65535), the column tiles the x axis, the coefficient launch is
// one thread per entry, and every tensor must have a byte size
static int l1_limits(const char* who, int R, int N, int64_t K) {
    if ((R + L1_RR - 1) / L1_RR > 65535) return fail(KCCOT_EUNSUPPORTED, "%s: %d target rows > %d", who, R, 65535 * L1_RR);
    if ((K + L1_KT - 1) / L1_KT > 2147483647LL) return fail(KCCOT_EUNSUPPORTED, "%s: K=%lld too large", who, (long long)K);
    if (((int64_t)N * l1_pad(R) + 255) / 256 > 2147483647LL)
        return fail(KCCOT_EUNSUPPORTED, "%s: a %d x %d coefficient matrix is too large", who, R, N);
    const int mx = R > N ? R : N;
    if (K > (int64_t)1 << 40 || (int64_t)mx * K > (int64_t)1 << 59)
        return fail(KCCOT_EUNSUPPORTED, "%s: a [%d, %lld] tensor is too large", who, mx, (long long)K);
    return 0;
}

// out [R,K] = sc * sum_c W[r,c] sgn(a[r,k] - S[c,k]); sources S1 [n1,K] then S2 [n2,K] (n2 may be 0); g as l1_build_coeffs
static int l1_job(int mode, const float* g, int Bx, int By, const float* a, int R, const float* S1, int n1, const float* S2,
                  int n2, int64_t K, float sc, float* out, float* Wt, hipStream_t st) {
    const int N = n1 + n2, Rp = l1_pad(R);
    hipLaunchKernelGGL(l1_build_coeffs, dim3((unsigned)(((int64_t)N * Rp + 255) / 256)), dim3(256), 0, st, mode, g, Bx, By, R, Rp,
                       N, Wt);
    if (int rc = launch_status("l1_build_coeffs")) return rc;
    const uintptr_t bits = (uintptr_t)a | (uintptr_t)S1 | (uintptr_t)(n2 ? S2 : S1) | (uintptr_t)out;
    const bool vec = K % 4 == 0 && bits % 16 == 0;
    const dim3 grid((unsigned)((K + L1_KT - 1) / L1_KT), (unsigned)(Rp / L1_RR));
    if (vec) hipLaunchKernelGGL(l1_sign_apply<true>, grid, dim3(L1_NT), 0, st, a, S1, n1, S2, n2, (const float*)Wt, R, Rp, K, sc, out);
    else hipLaunchKernelGGL(l1_sign_apply<false>, grid, dim3(L1_NT), 0, st, a, S1, n1, S2, n2, (const float*)Wt, R, Rp, K, sc, out);
    return launch_status("l1_sign_apply");
}

}  // namespace kccot

using namespace kccot;

extern "C" size_t kccot_l1_cost_bwd_workspace_bytes(int Bx, int By) {
    if (Bx <= 0 || By <= 0) return 0;
    return l1_coef_bytes(Bx, By) + l1_coef_bytes(By, Bx);       // dx's [By][pad Bx], then dy's [Bx][pad By]
}

extern "C" int kccot_l1_cost_bwd_f32(const float* g, const float* x, const float* y, int Bx, int By, int64_t K, float sc,
                                     unsigned flags, float* dx, float* dy, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const char* who = "l1_cost_bwd";
    if (!g || !x || !y) return fail(KCCOT_EINVAL, "%s: null input pointer", who);
    if (!dx && !dy) return fail(KCCOT_EINVAL, "%s: null output pointers (give dx, dy or both)", who);
    if (Bx <= 0 || By <= 0 || K <= 0)
        return fail(KCCOT_EINVAL, "%s: bad shape Bx=%d By=%d K=%lld", who, Bx, By, (long long)K);
    if (flags & ~KCCOT_COST_SAME) return fail(KCCOT_EINVAL, "%s: unknown flags 0x%x (0 or KCCOT_COST_SAME)", who, flags);
    const bool same = (flags & KCCOT_COST_SAME) != 0;
    if (same && (x != y || Bx != By || dy))
        return fail(KCCOT_EINVAL, "%s: KCCOT_COST_SAME needs x == y, Bx == By and dy == NULL", who);
    if (int rc = l1_limits(who, Bx > By ? Bx : By, Bx > By ? Bx : By, K)) return rc;
    const size_t gb = (size_t)Bx * By * sizeof(float), xb = (size_t)Bx * K * sizeof(float), yb = (size_t)By * K * sizeof(float);
    if (l1_overlap(dx, xb, g, gb) || l1_overlap(dx, xb, x, xb) || l1_overlap(dx, xb, y, yb) || l1_overlap(dy, yb, g, gb) ||
        l1_overlap(dy, yb, x, xb) || l1_overlap(dy, yb, y, yb) || l1_overlap(dx, xb, dy, yb))
        return fail(KCCOT_EINVAL, "%s: an output must not alias an input or the other output", who);
    const size_t need = kccot_l1_cost_bwd_workspace_bytes(Bx, By);
    if (!ws || ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", who, ws_bytes, need);
    const hipStream_t st = (hipStream_t)stream;
    float* W1 = static_cast<float*>(ws);
    float* W2 = reinterpret_cast<float*>(static_cast<char*>(ws) + l1_coef_bytes(Bx, By));
    if (same) return l1_job(L1_SAME, g, Bx, By, x, Bx, x, Bx, nullptr, 0, K, sc, dx, W1, st);
    if (dx)
        if (int rc = l1_job(L1_DX, g, Bx, By, x, Bx, y, By, nullptr, 0, K, sc, dx, W1, st)) return rc;
    if (dy)
        if (int rc = l1_job(L1_DY, g, Bx, By, y, By, x, Bx, nullptr, 0, K, sc, dy, W2, st)) return rc;
    return 0;
}

extern "C" size_t kccot_l1_cost3_bwd_workspace_bytes(int B) {
    if (B <= 0) return 0;
    return l1_coef_bytes(B, 2 * B);
}

extern "C" int kccot_l1_cost3_bwd_f32(const float* g3, const float* real, const float* fake, int B, int64_t K, float sc,
                                      float* dfake, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    const char* who = "l1_cost3_bwd";
    if (!g3 || !real || !fake) return fail(KCCOT_EINVAL, "%s: null input pointer", who);
    if (!dfake) return fail(KCCOT_EINVAL, "%s: null output pointer", who);
    if (B <= 0 || K <= 0) return fail(KCCOT_EINVAL, "%s: bad shape B=%d K=%lld", who, B, (long long)K);
    if (B > (1 << 30)) return fail(KCCOT_EUNSUPPORTED, "%s: %d target rows > %d", who, B, 65535 * L1_RR);
    if (int rc = l1_limits(who, B, 2 * B, K)) return rc;
    const size_t gb = (size_t)3 * B * B * sizeof(float), vb = (size_t)B * K * sizeof(float);
    if (l1_overlap(dfake, vb, g3, gb) || l1_overlap(dfake, vb, real, vb) || l1_overlap(dfake, vb, fake, vb))
        return fail(KCCOT_EINVAL, "%s: dfake must not alias an input", who);
    const size_t need = kccot_l1_cost3_bwd_workspace_bytes(B);
    if (!ws || ws_bytes < need) return fail(KCCOT_EWORKSPACE, "%s: workspace %zu < required %zu", who, ws_bytes, need);
    return l1_job(L1_LOSS, g3, B, B, fake, B, real, B, fake, B, K, sc, dfake, static_cast<float*>(ws), (hipStream_t)stream);
}
