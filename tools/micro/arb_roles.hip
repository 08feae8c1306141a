// Who gets a SIMD's vector port when a dependent chain and an independent block of VALU work share it?  One 1024-thread
// workgroup (four waves per SIMD): waves 0-7 and waves 8-15 are two groups on the same SIMDs, two waves of each per SIMD.
// Between two barriers group A runs the chain pass of the reverse Sinkhorn sweep (4 v_pk_mul_f32, 8 serial v_add_f32, the
// 3-step DPP sum with its hazard slots) and group B the plan pass (8 x v_sub_f32, v_add_f32, v_exp_f32).  A's segment is
// timed with the shader clock, the whole loop with one clock pair, in three cases: A = the older waves, A = the younger
// waves, A = the younger waves at s_setprio 1 for the segment; and A alone (B idle at the barrier) as the floor.
//   hipcc --offload-arch=gfx950 -O3 tools/micro/arb_roles.hip -o /tmp/arb_roles && /tmp/arb_roles
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void chain_mix(f32x2 (&p)[4], const f32x2 (&pl)[4], const f32x2 (&g)[4], float& s) {
    asm volatile("v_pk_mul_f32 %0, %4, %8\n\tv_pk_mul_f32 %1, %5, %9\n\tv_pk_mul_f32 %2, %6, %10\n\tv_pk_mul_f32 %3, %7, %11"
                 : "=&v"(p[0]), "=&v"(p[1]), "=&v"(p[2]), "=&v"(p[3])
                 : "v"(pl[0]), "v"(pl[1]), "v"(pl[2]), "v"(pl[3]), "v"(g[0]), "v"(g[1]), "v"(g[2]), "v"(g[3]));
    asm volatile(
        "v_add_f32 %0, 0, %1\n\tv_add_f32 %0, %0, %2\n\tv_add_f32 %0, %0, %3\n\tv_add_f32 %0, %0, %4\n\t"
        "v_add_f32 %0, %0, %5\n\tv_add_f32 %0, %0, %6\n\tv_add_f32 %0, %0, %7\n\tv_add_f32 %0, %0, %8\n\t"
        "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
        "s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1"
        : "=&v"(s)
        : "v"(p[0].x), "v"(p[0].y), "v"(p[1].x), "v"(p[1].y), "v"(p[2].x), "v"(p[2].y), "v"(p[3].x), "v"(p[3].y));
}
__device__ __forceinline__ void plan_mix(float (&e)[8], const float (&c)[8], float sv, float o) {
#pragma unroll
    for (int m = 0; m < 8; ++m)
        asm volatile("v_sub_f32 %0, %1, %2\n\tv_add_f32 %0, %0, %3\n\tv_exp_f32 %0, %0" : "=&v"(e[m]) : "v"(sv), "v"(c[m]), "v"(o));
#pragma unroll
    for (int m = 0; m < 8; ++m) asm volatile("" :: "v"(e[m]));        // eight live results, as the pinned plan has
}

// A_YOUNG: group A is waves 8-15; PRIO: A's segment runs at s_setprio 1; B_ON: group B works (else it waits at the barrier)
template <bool A_YOUNG, bool PRIO, bool B_ON>
__global__ __launch_bounds__(1024) void k(unsigned long long* out, float* sink, int iters) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const bool is_a = (wave >= 8) == A_YOUNG;
    float c[8], e[8], s = 0.f, acc = 0.f;
    f32x2 g[4], pl[4], p[4];
    for (int m = 0; m < 8; ++m) { c[m] = 0.5f * m; e[m] = 0.f; }
    for (int m = 0; m < 4; ++m) { g[m] = 1.0f + 0.001f * (threadIdx.x + m); pl[m] = 0.25f + 0.01f * m; p[m] = 0.f; }
    unsigned long long seg = 0;
    __syncthreads();
    const unsigned long long t_begin = __builtin_amdgcn_s_memtime();
    if (is_a) {
        for (int it = 0; it < iters; ++it) {
            __builtin_amdgcn_s_barrier();
            const unsigned long long t0 = __builtin_amdgcn_s_memtime();
            if (PRIO) __builtin_amdgcn_s_setprio(1);
            chain_mix(p, pl, g, s);
            if (PRIO) __builtin_amdgcn_s_setprio(0);
            asm volatile("s_nop 4" :: "v"(s));                         // the clock is read once the sum exists
            seg += __builtin_amdgcn_s_memtime() - t0;
            acc += s + p[0].x + p[3].y;
            __builtin_amdgcn_s_barrier();
        }
    } else {
        for (int it = 0; it < iters; ++it) {
            __builtin_amdgcn_s_barrier();
            if (B_ON) { plan_mix(e, c, g[0].x, g[1].x); acc += e[0] + e[7]; }
            __builtin_amdgcn_s_barrier();
        }
    }
    const unsigned long long t_end = __builtin_amdgcn_s_memtime();
    if ((threadIdx.x & 63) == 0) { out[wave * 2] = seg; out[wave * 2 + 1] = t_end - t_begin; }
    sink[threadIdx.x] = acc;
}

template <bool A_YOUNG, bool PRIO, bool B_ON>
static void run(const char* what, unsigned long long* out, float* sink, int iters) {
    unsigned long long h[32];
    for (int rep = 0; rep < 3; ++rep) {                                // the last launch is reported
        hipLaunchKernelGGL((k<A_YOUNG, PRIO, B_ON>), dim3(1), dim3(1024), 0, 0, out, sink, iters);
        if (hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) { printf("%s: launch failed\n", what); return; }
    }
    double seg = 0, loop = 0;
    for (int w = 0; w < 16; ++w) { if ((w >= 8) == A_YOUNG) seg += h[w * 2]; loop += h[w * 2 + 1]; }
    printf("%-44s A's segment %7.1f cycles   one iteration (two barriers) %7.1f cycles\n", what, seg / 8 / iters, loop / 16 / iters);
}

int main() {
    unsigned long long* out; float* sink;
    if (hipMalloc(&out, 32 * sizeof(unsigned long long)) != hipSuccess || hipMalloc(&sink, 1024 * sizeof(float)) != hipSuccess) return 1;
    const int iters = 20000;
    run<false, false, false>("A older, B idle (floor)", out, sink, iters);
    run<true, false, false>("A younger, B idle (floor)", out, sink, iters);
    run<false, false, true>("A older, B works, both priority 0", out, sink, iters);
    run<true, false, true>("A younger, B works, both priority 0", out, sink, iters);
    run<true, true, true>("A younger at s_setprio 1, B works", out, sink, iters);
    run<false, true, true>("A older at s_setprio 1, B works", out, sink, iters);
    (void)hipFree(out); (void)hipFree(sink);
    return 0;
}
