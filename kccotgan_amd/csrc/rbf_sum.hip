// KCCOT_COST_RBF_SUM (kccot_pairwise_cost_f32): a finished block of squared distances C [Bx,By] becomes the Gaussian kernel
// block exp(-sc * C) in place, and the fp64 sum of its entries is left as ONE double at the start of the workspace -- the
// per-rank piece of the batch-sharded kernel-MMD (kccotgan_amd/dist.py, sharded_rbf_mmd2): every rank turns its three
// [B/G, B] row blocks into kernel values, the 3 sums are all-reduced, mmd^2 = (Sxx + Syy - 2 Sxy) / B^2.
// An extension with no reference behaviour, as kccot_rbf_mmd_f32 (martingale.hip), whose one-workgroup kernel takes the
// whole [3,B,B] on one CU; each entry here is the same expression, expf(-gamma * d), so the kernel values of equal
// distances are equal bit for bit.
//
// Two launches, no atomics, a fixed summation order (two calls and a graph replay give the same bits):
//   rbf_sum_tiles    grid (ceil(By / 64), ceil(Bx / 4)), one wave per 4 x 64 tile ([64,512]: 128 workgroups).  Rows that are
//                    16-byte aligned (base aligned and By % 4 == 0): lane l owns row l / 16, columns 4 (l % 16) .. + 3 as one
//                    float4; otherwise lane l owns column l of each of the 4 rows (scalar, coalesced).  The lane's four
//                    values are added in fp64 in ascending order, the wave's by the xor butterfly; lane 0 stores the
//                    tile's partial at ws[1 + tile] with a plain (vector) store.
//   rbf_sum_combine  one workgroup: thread t adds the partials t, t + 256, ... in ascending order, the waves' sums meet in
//                    LDS and thread 0 adds them in wave order and stores ws[0].
#include "common.h"
#include <math.h>

namespace kccot {

constexpr int RS_ROWS = 4;     // tile rows
constexpr int RS_COLS = 64;    // tile columns

__global__ __launch_bounds__(64) void rbf_sum_tiles(float* __restrict__ C, int Bx, int By, float gamma, int vec,
                                                    double* __restrict__ partial) {
    const int lane = threadIdx.x;
    const int i0 = blockIdx.y * RS_ROWS, j0 = blockIdx.x * RS_COLS;
    double s = 0.0;
    if (vec) {
        const int i = i0 + (lane >> 4), j = j0 + 4 * (lane & 15);
        if (i < Bx && j < By) {          // By % 4 == 0: the float4 lies inside the row or outside it
            float4* p = reinterpret_cast<float4*>(C + (int64_t)i * By + j);
            const float4 d = *p;
            float4 k;
            k.x = expf(-gamma * d.x);
            k.y = expf(-gamma * d.y);
            k.z = expf(-gamma * d.z);
            k.w = expf(-gamma * d.w);
            *p = k;
            s = (((double)k.x + (double)k.y) + (double)k.z) + (double)k.w;
        }
    } else {
        const int j = j0 + lane;
        if (j < By) {
#pragma unroll
            for (int r = 0; r < RS_ROWS; ++r) {
                const int i = i0 + r;
                if (i < Bx) {
                    float* p = C + (int64_t)i * By + j;
                    const float k = expf(-gamma * *p);
                    *p = k;
                    s += (double)k;
                }
            }
        }
    }
    s = wave_sum_d(s);
    if (lane == 0) partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void rbf_sum_combine(const double* __restrict__ partial, int64_t n, double* __restrict__ out) {
    __shared__ double part[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    double s = 0.0;
    for (int64_t e = threadIdx.x; e < n; e += 256) s += partial[e];
    s = wave_sum_d(s);
    if (lane == 0) part[wid] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = ((part[0] + part[1]) + part[2]) + part[3];
}

// doubles the call touches: the sum and one partial per tile
size_t rbf_sum_doubles(int Bx, int By) {
    return 1 + (size_t)((Bx + RS_ROWS - 1) / RS_ROWS) * (size_t)((By + RS_COLS - 1) / RS_COLS);
}

int launch_rbf_sum(float* C, int Bx, int By, float gamma, double* ws, hipStream_t st) {
    const unsigned gx = (unsigned)((By + RS_COLS - 1) / RS_COLS), gy = (unsigned)((Bx + RS_ROWS - 1) / RS_ROWS);
    const int vec = (By % 4 == 0) && ((uintptr_t)C % 16 == 0);
    hipLaunchKernelGGL(rbf_sum_tiles, dim3(gx, gy), dim3(64), 0, st, C, Bx, By, gamma, vec, ws + 1);
    int rc = launch_status("rbf_sum_tiles");
    if (rc) return rc;
    hipLaunchKernelGGL(rbf_sum_combine, dim3(1), dim3(256), 0, st, (const double*)(ws + 1), (int64_t)gx * gy, ws);
    return launch_status("rbf_sum_combine");
}

}  // namespace kccot
