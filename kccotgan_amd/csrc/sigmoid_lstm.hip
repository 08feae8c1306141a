// The discriminators' last layer, Keras LSTM(units, activation='sigmoid') (kccot_sigmoid_lstm_{fwd,bwd}_f32,
// include/kccot_models.h): the whole recurrence over T as ONE launch each way instead of a dozen tensor-op launches per
// step.  The work is tiny (U = 8 units, 64 samples at BASELINE configs[1]) and serial in t, so the kernel is built for
// the latency of one step, not for throughput.
//
// Mapping: a group of P = pow2ceil(U) lanes owns one sample, 64 / P samples share a wave, one wave per workgroup.  Lane k
// of a group owns unit k: its four gate rows of wh, its c, its h.  h (forward) and dg (backward) travel inside the group
// by ds_bpermute (__shfl with width P); a sample never leaves its wave, so there is no barrier in the time loop and no
// atomic anywhere.  Every sum runs j = 0..U-1 in order within the owning lane: a sample's bits depend on its own inputs
// and wh only, not on B or on where the sample sits.
//   P <= 16: the lane's rows of wh (and, backward, its column) live in registers, padded with zeros to P.
//   P >= 32: wh sits in LDS, transposed and XOR-swizzled so that both access patterns (lanes along the rows for the
//            gates, lanes along the columns for wh^T dg) are free of bank conflicts.  At most 64 KiB (U = 64).
// Backward recomputes the gates from gx and h_{t-1} (h_seq) with the forward's own expression -- off the serial chain:
// nothing of it depends on the carries -- instead of reading 4U saved floats per step.
// The loads of step t +- 2 are issued before step t is worked on (the serial chain of a step is shorter than an L2 miss).
#include "common.h"
#include "../../include/kccot_models.h"

namespace kccot {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int P>
struct WhLds {                          // wh [4U,U] as lds[j * S + (r ^ (j & 31))], r = gate row, j = column
    static constexpr int S = 4 * P;     // a multiple of 32: the swizzle stays inside the row
    float* lds;
    __device__ __forceinline__ void fill(const float* __restrict__ wh, int U, int lane) {
        for (int e = lane; e < 4 * U * U; e += 64) {
            const int r = e / U, j = e - r * U;
            lds[j * S + (r ^ (j & 31))] = wh[e];
        }
        __syncthreads();
    }
    __device__ __forceinline__ float at(int r, int j) const { return lds[j * S + (r ^ (j & 31))]; }
};

// g[q] += sum_j wh[q U + k, j] h_j, j ascending; h_j is lane j's value of the group
template <int P>
__device__ __forceinline__ void add_recurrent(float (&g)[4], float h, const float (&wr)[4][P <= 16 ? P : 1], const WhLds<P>& wl,
                                              int kk, int U) {
    if constexpr (P <= 16) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
            const float hj = __shfl(h, j, P);
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = fmaf(wr[q][j], hj, g[q]);
        }
    } else {
        for (int j = 0; j < U; ++j) {
            const float hj = __shfl(h, j, P);
#pragma unroll
            for (int q = 0; q < 4; ++q) g[q] = fmaf(wl.at(q * U + kk, j), hj, g[q]);
        }
    }
}

template <int P>
__global__ __launch_bounds__(64) void sigmoid_lstm_fwd(const float* __restrict__ gx, const float* __restrict__ wh, int B, int T, int U,
                                                       float* __restrict__ h_seq, float* __restrict__ c_seq) {
    constexpr bool REGS = P <= 16;
    __shared__ float lds[REGS ? 1 : 4 * P * P];
    const int lane = threadIdx.x, k = lane & (P - 1), kk = k < U ? k : U - 1;
    const int64_t b = (int64_t)blockIdx.x * (64 / P) + lane / P;
    const bool live = b < B && k < U;                  // dead lanes run along (the shuffles need them) and touch no memory
    float wr[4][REGS ? P : 1];
    WhLds<P> wl{lds};
    if constexpr (REGS) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < P; ++j) wr[q][j] = (k < U && j < U) ? wh[(q * U + k) * U + j] : 0.f;
    } else {
        wl.fill(wh, U, lane);
    }
    const int64_t U4 = 4 * (int64_t)U;
    const int64_t gb = b * T * U4 + k, ob = b * T * U + k;
    auto load = [&](float (&d)[4], int t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) d[q] = (live && t < T) ? gx[gb + t * U4 + q * U] : 0.f;
    };
    float pa[4], pb[4], g[4];
    load(pa, 0);
    load(pb, 1);
    float h = 0.f, c = 0.f;
    for (int t = 0; t < T; ++t) {
#pragma unroll
        for (int q = 0; q < 4; ++q) { g[q] = pa[q]; pa[q] = pb[q]; }
        load(pb, t + 2);
        add_recurrent<P>(g, h, wr, wl, kk, U);
        c = sigm(g[1]) * c + sigm(g[0]) * sigm(g[2]);
        h = k < U ? sigm(g[3]) * sigm(c) : 0.f;
        if (live) {
            h_seq[ob + (int64_t)t * U] = h;
            if (c_seq) c_seq[ob + (int64_t)t * U] = c;
        }
    }
}

struct BwdStep { float g[4], hp, cp, dh; };             // gx_t, h_{t-1}, c_{t-1}, upstream dh_t of one unit

template <int P>
__global__ __launch_bounds__(64) void sigmoid_lstm_bwd(const float* __restrict__ gx, const float* __restrict__ wh,
                                                       const float* __restrict__ h_seq, const float* __restrict__ c_seq,
                                                       const float* __restrict__ dh_seq, int B, int T, int U, float* __restrict__ dgx) {
    constexpr bool REGS = P <= 16;
    __shared__ float lds[REGS ? 1 : 4 * P * P];
    const int lane = threadIdx.x, k = lane & (P - 1), kk = k < U ? k : U - 1;
    const int64_t b = (int64_t)blockIdx.x * (64 / P) + lane / P;
    const bool live = b < B && k < U;
    float wr[4][REGS ? P : 1], wt[4][REGS ? P : 1];     // wr: the lane's gate rows; wt: its column, wt[q][j] = wh[q U + j, k]
    WhLds<P> wl{lds};
    if constexpr (REGS) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < P; ++j) {
                wr[q][j] = (k < U && j < U) ? wh[(q * U + k) * U + j] : 0.f;
                wt[q][j] = (k < U && j < U) ? wh[(q * U + j) * U + k] : 0.f;
            }
    } else {
        wl.fill(wh, U, lane);
    }
    const int64_t U4 = 4 * (int64_t)U;
    const int64_t gb = b * T * U4 + k, ob = b * T * U + k;
    auto load = [&](BwdStep& s, int t) {
        const bool on = live && t >= 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) s.g[q] = on ? gx[gb + t * U4 + q * U] : 0.f;
        s.dh = on ? dh_seq[ob + (int64_t)t * U] : 0.f;
        s.hp = (on && t > 0) ? h_seq[ob + (int64_t)(t - 1) * U] : 0.f;
        s.cp = (on && t > 0) ? c_seq[ob + (int64_t)(t - 1) * U] : 0.f;
    };
    BwdStep pa, pb, s;
    load(pa, T - 1);
    load(pb, T - 2);
    float ct = live ? c_seq[ob + (int64_t)(T - 1) * U] : 0.f;
    float dh_carry = 0.f, dc_carry = 0.f;               // wh^T dg_{t+1} and dc_{t+1} f_{t+1}
    for (int t = T - 1; t >= 0; --t) {
        s = pa;
        pa = pb;
        load(pb, t - 2);
        add_recurrent<P>(s.g, s.hp, wr, wl, kk, U);
        const float i = sigm(s.g[0]), f = sigm(s.g[1]), cc = sigm(s.g[2]), o = sigm(s.g[3]), sc = sigm(ct);
        const float dh = s.dh + dh_carry;
        const float dc = dc_carry + dh * o * (sc * (1.f - sc));
        float dg[4];
        dg[0] = dc * cc * (i * (1.f - i));
        dg[1] = dc * s.cp * (f * (1.f - f));
        dg[2] = dc * i * (cc * (1.f - cc));
        dg[3] = dh * sc * (o * (1.f - o));
        dc_carry = dc * f;
        ct = s.cp;
        if (live) {
#pragma unroll
            for (int q = 0; q < 4; ++q) dgx[gb + t * U4 + q * U] = dg[q];
        }
        if (t == 0) break;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};            // lane k: sum_q sum_j wh[q U + j, k] dg_q[j], j ascending per gate
        if constexpr (REGS) {
#pragma unroll
            for (int j = 0; j < P; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(wt[q][j], __shfl(k < U ? dg[q] : 0.f, j, P), acc[q]);
        } else {
            for (int j = 0; j < U; ++j)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[q] = fmaf(wl.at(q * U + j, kk), __shfl(dg[q], j, P), acc[q]);
        }
        dh_carry = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    }
}

static int pow2ceil(int u) {
    int p = 1;
    while (p < u) p <<= 1;
    return p;
}

}  // namespace kccot
using namespace kccot;

#define KCCOT_SLSTM_DISPATCH(KERNEL, ...)                                                                                  \
    switch (P) {                                                                                                           \
        case 1: hipLaunchKernelGGL(KERNEL<1>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                            \
        case 2: hipLaunchKernelGGL(KERNEL<2>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                            \
        case 4: hipLaunchKernelGGL(KERNEL<4>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                            \
        case 8: hipLaunchKernelGGL(KERNEL<8>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                            \
        case 16: hipLaunchKernelGGL(KERNEL<16>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                          \
        case 32: hipLaunchKernelGGL(KERNEL<32>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                          \
        default: hipLaunchKernelGGL(KERNEL<64>, dim3(grid), dim3(64), 0, st, __VA_ARGS__); break;                          \
    }

extern "C" int kccot_sigmoid_lstm_fwd_f32(const float* gx, const float* wh, int B, int T, int U, float* h_seq, float* c_seq,
                                          kccot_stream_t stream) {
    if (!gx || !wh || !h_seq) return fail(KCCOT_EINVAL, "sigmoid_lstm_fwd: null pointer");
    if (B <= 0 || T <= 0 || U <= 0) return fail(KCCOT_EINVAL, "sigmoid_lstm_fwd: bad shape B=%d T=%d U=%d", B, T, U);
    if (U > 64) return fail(KCCOT_EUNSUPPORTED, "sigmoid_lstm_fwd: U=%d units (at most 64)", U);
    const int P = pow2ceil(U);
    const unsigned grid = (unsigned)(((int64_t)B + 64 / P - 1) / (64 / P));
    hipStream_t st = (hipStream_t)stream;
    KCCOT_SLSTM_DISPATCH(sigmoid_lstm_fwd, gx, wh, B, T, U, h_seq, c_seq)
    return launch_status("sigmoid_lstm_fwd");
}

extern "C" int kccot_sigmoid_lstm_bwd_f32(const float* gx, const float* wh, const float* h_seq, const float* c_seq,
                                          const float* dh_seq, int B, int T, int U, float* dgx, kccot_stream_t stream) {
    if (!gx || !wh || !h_seq || !c_seq || !dh_seq || !dgx) return fail(KCCOT_EINVAL, "sigmoid_lstm_bwd: null pointer");
    if (B <= 0 || T <= 0 || U <= 0) return fail(KCCOT_EINVAL, "sigmoid_lstm_bwd: bad shape B=%d T=%d U=%d", B, T, U);
    if (U > 64) return fail(KCCOT_EUNSUPPORTED, "sigmoid_lstm_bwd: U=%d units (at most 64)", U);
    const int P = pow2ceil(U);
    const unsigned grid = (unsigned)(((int64_t)B + 64 / P - 1) / (64 / P));
    hipStream_t st = (hipStream_t)stream;
    KCCOT_SLSTM_DISPATCH(sigmoid_lstm_bwd, gx, wh, h_seq, c_seq, dh_seq, B, T, U, dgx)
    return launch_status("sigmoid_lstm_bwd");
}
