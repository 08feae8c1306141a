// fp32 products on the bf16 matrix pipe, exactly: the three-way split and its six-product MFMA chain (DESIGN.md section 4,
// "Shared arithmetic (ii)").  The matrix-pipe kernels of the cost path (cost_mfma.hip, cost_tiled.hip, cost_tile256.hip,
// cost_rows.hip, cost_bwd.hip, cost_bwd_q256.hip) are built from these pieces; the one chain still spelled out elsewhere is
// the KCCOT_A4 macro of apply_coeffs_x3_m256 (cost_bwd.hip), see the note at KCCOT_MFMA_X3_2X2.
//
// Every fp32 value is cut into three bf16 pieces by truncation, x = h + m + l exactly (8 + 8 + 8 significand bits: h = top
// half of the word, m = top half of x - h, l = x - h - m), while a tile is staged; a product sum is accumulated in fp32 as
//     sum_k  xh*yh + (xh*ym + xm*yh) + (xh*yl + xl*yh + xm*ym)
// -- six v_mfma_f32_32x32x16_bf16 per 16 k instead of eight v_mfma_f32_32x32x2_f32, each of them four times shorter in issue
// cycles per k.  bf16 x bf16 products are exact in fp32; the dropped terms xm*yl + xl*ym + xl*yl are below 2^-24 of |x*y|,
// i.e. under the rounding of the fp32 accumulation itself, so this is fp32 arithmetic to working precision (parity tests
// run the bf16 and the f32-input kernels against the same golden vectors).
//
// The ORDER of the six products (smallest terms first: mm, hl, lh, hm, mh, hh) is a numerical contract: it is what makes
// the kernels that share it bit-identical to each other (fused vs staged, apply_q256 vs the tile kernels, rows vs full).
// It is written down in mfma_x3, KCCOT_MFMA_X3_2X2 and mfma_x3_tiles below.
#pragma once
#include "common.h"

namespace kccot {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// MFMA operand of one 32-row block and one 16-k step, lane l holding row (l & 31), k-half (l >> 5): the three pieces
struct Frag3 { bf16x8 h, m, l; };

// Accumulator register r of lane l of a 32 x 32 MFMA tile is element (acc_row(r) + 4 * (l >> 5), l & 31)
__device__ __forceinline__ constexpr int acc_row(int r) { return (r & 3) + 8 * (r >> 2); }

// ---- split and pack ------------------------------------------------------------------------------------------------
// the pieces are the UPPER 16 bits of the words h, m, l
// x minus its top bf16 piece: exact, and 8 significant bits shorter
__device__ __forceinline__ float bf16_rest(float x) { return x - __uint_as_float(__float_as_uint(x) & 0xFFFF0000u); }

__device__ __forceinline__ void split3u(float x, unsigned& h, unsigned& m, unsigned& l) {
    const float r1 = bf16_rest(x), r2 = bf16_rest(r1);
    h = __float_as_uint(x); m = __float_as_uint(r1); l = __float_as_uint(r2);
}

// dword = bf16(a) | bf16(b) << 16 from the words of a and b (v_perm)
__device__ __forceinline__ unsigned bf16_pair(unsigned a, unsigned b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }

// the word pairs (a, b) of the three pieces -> one dword per plane at off, plane + off, 2 plane + off
__device__ __forceinline__ void store_pairs3(unsigned char* zs, int64_t plane, int off, unsigned ha, unsigned hb, unsigned ma,
                                             unsigned mb, unsigned la, unsigned lb) {
    *reinterpret_cast<unsigned*>(zs + off) = bf16_pair(ha, hb);
    *reinterpret_cast<unsigned*>(zs + plane + off) = bf16_pair(ma, mb);
    *reinterpret_cast<unsigned*>(zs + 2 * plane + off) = bf16_pair(la, lb);
}

// two floats -> the same; the two splits advance side by side (the order the every-wave-stages kernels were scheduled with)
__device__ __forceinline__ void split3_store2(unsigned char* zs, int64_t plane, int off, float a, float b) {
    const float ra = bf16_rest(a), rb = bf16_rest(b);
    const float la = bf16_rest(ra), lb = bf16_rest(rb);
    store_pairs3(zs, plane, off, __float_as_uint(a), __float_as_uint(b), __float_as_uint(ra), __float_as_uint(rb),
                 __float_as_uint(la), __float_as_uint(lb));
}

// four consecutive floats -> 8 bytes per plane
__device__ __forceinline__ void split3_pack4(float4 v, uint2& ph, uint2& pm, uint2& pl) {
    const float x[4] = {v.x, v.y, v.z, v.w};
    unsigned h[4], m[4], l[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) split3u(x[i], h[i], m[i], l[i]);
    ph.x = bf16_pair(h[0], h[1]); ph.y = bf16_pair(h[2], h[3]);
    pm.x = bf16_pair(m[0], m[1]); pm.y = bf16_pair(m[2], m[3]);
    pl.x = bf16_pair(l[0], l[1]); pl.y = bf16_pair(l[2], l[3]);
}

__device__ __forceinline__ void split3_store4(unsigned char* zs, int64_t plane, int off, float4 v) {
    uint2 ph, pm, pl;
    split3_pack4(v, ph, pm, pl);
    *reinterpret_cast<uint2*>(zs + off) = ph;
    *reinterpret_cast<uint2*>(zs + plane + off) = pm;
    *reinterpret_cast<uint2*>(zs + 2 * plane + off) = pl;
}

// ---- fragment loads: three planes `plane` bytes apart -----------------------------------------------------------------
__device__ __forceinline__ Frag3 ld_frag3(const unsigned char* zs, int64_t plane, int off) {      // 16-byte reads
    Frag3 f;
    f.h = *reinterpret_cast<const bf16x8*>(zs + off);
    f.m = *reinterpret_cast<const bf16x8*>(zs + plane + off);
    f.l = *reinterpret_cast<const bf16x8*>(zs + 2 * plane + off);
    return f;
}

// one piece as two 8-byte halves, for stages whose rows are 8- but not 16-byte aligned (ds_read_b64 x 2)
__device__ __forceinline__ bf16x8 ld_piece_b64(const unsigned char* p) {
    bf16x8 v;
    uint2* q = reinterpret_cast<uint2*>(&v);
    q[0] = *reinterpret_cast<const uint2*>(p);
    q[1] = *reinterpret_cast<const uint2*>(p + 8);
    return v;
}
__device__ __forceinline__ Frag3 ld_frag3_b64(const unsigned char* zs, int64_t plane, int off) {
    Frag3 f;
    f.h = ld_piece_b64(zs + off);
    f.m = ld_piece_b64(zs + plane + off);
    f.l = ld_piece_b64(zs + 2 * plane + off);
    return f;
}

// ---- product chains -----------------------------------------------------------------------------------------------------
// One 32 x 32 accumulator tile.  (KCCOT_ABLATE_MFMA16: the TIMING-ONLY build of tools/micro/q256_mfma16_ablate.sh -- results are
// garbage -- keeps it as four 16 x 16 quarter tiles and issues twelve v_mfma_f32_16x16x32_bf16 per fragment pair: the same FLOPs,
// operand reads and registers; does the shape's higher sustained clock (tools/micro/mfma_shape.hip) survive next to the
// kernels' LDS and VALU traffic?)
#ifdef KCCOT_ABLATE_MFMA16
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct X3Acc { f32x4 q[4]; };
#define X3ACC(a, r) (a).q[(r) >> 2][(r) & 3]
__device__ __forceinline__ void mfma_x3(X3Acc& acc, const Frag3& a, const Frag3& b) {
    acc.q[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, acc.q[0], 0, 0, 0);
    acc.q[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.m, acc.q[1], 0, 0, 0);
    acc.q[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, acc.q[2], 0, 0, 0);
    acc.q[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.l, acc.q[3], 0, 0, 0);
    acc.q[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, acc.q[0], 0, 0, 0);
    acc.q[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.l, b.h, acc.q[1], 0, 0, 0);
    acc.q[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, acc.q[2], 0, 0, 0);
    acc.q[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.m, acc.q[3], 0, 0, 0);
    acc.q[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, acc.q[0], 0, 0, 0);
    acc.q[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.m, b.h, acc.q[1], 0, 0, 0);
    acc.q[2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, acc.q[2], 0, 0, 0);
    acc.q[3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.h, b.h, acc.q[3], 0, 0, 0);
}
#else
typedef f32x16 X3Acc;
#define X3ACC(a, r) (a)[r]
#endif

// acc += A * B^T:  hh + (hm + mh) + (hl + lh + mm), smallest terms first
__device__ __forceinline__ void mfma_x3(f32x16& acc, const Frag3& a, const Frag3& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.l, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.l, b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.m, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.m, b.h, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.h, b.h, acc, 0, 0, 0);
}

// A diagonal sub-tile (A = B = F) is symmetric: S += mm + hh (symmetric products), A += hl + hm (their transposes are the
// two products left out); the caller forms S + A + A^T
__device__ __forceinline__ void mfma_x3_diag(f32x16& accS, f32x16& accA, const Frag3& f) {
    accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.m, f.m, accS, 0, 0, 0);
    accA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.h, f.l, accA, 0, 0, 0);
    accA = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.h, f.m, accA, 0, 0, 0);
    accS = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.h, f.h, accS, 0, 0, 0);
}

// The same chain over 2 x 2 accumulator tiles (rows A0, A1 x columns B0, B1) in PRODUCT-MAJOR order: the four accumulators
// take turns, so no MFMA waits on the one issued before it; per accumulator the order is mfma_x3's.  (A macro: as a function
// taking the eight operands by reference it compiled to a different schedule in cost_tiled.hip.  apply_coeffs_x3_m256 keeps
// its own copy: through this macro its schedule changed as well.  Figures: profiles/bf16x3_isa_identity.txt.)
#define KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, PA, PB)                \
    C00 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0.PA, B0.PB, C00, 0, 0, 0); \
    C01 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A0.PA, B1.PB, C01, 0, 0, 0); \
    C10 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1.PA, B0.PB, C10, 0, 0, 0); \
    C11 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A1.PA, B1.PB, C11, 0, 0, 0);
#define KCCOT_MFMA_X3_2X2(C00, C01, C10, C11, A0, A1, B0, B1)                                                         \
    KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, m, m) KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, h, l)       \
    KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, l, h) KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, h, m)       \
    KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, m, h) KCCOT_X3_P4(C00, C01, C10, C11, A0, A1, B0, B1, h, h)

// ... and over RT x CT tiles
template <int RT, int CT>
__device__ __forceinline__ void mfma_x3_tiles(f32x16 (&acc)[RT][CT], const Frag3 (&a)[RT], const Frag3 (&b)[CT]) {
#define KCCOT_X3_STEP(PA, PB)                                \
    _Pragma("unroll") for (int i = 0; i < RT; ++i)           \
        _Pragma("unroll") for (int j = 0; j < CT; ++j)       \
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i].PA, b[j].PB, acc[i][j], 0, 0, 0);
    KCCOT_X3_STEP(m, m) KCCOT_X3_STEP(h, l) KCCOT_X3_STEP(l, h) KCCOT_X3_STEP(h, m) KCCOT_X3_STEP(m, h) KCCOT_X3_STEP(h, h)
#undef KCCOT_X3_STEP
}

}  // namespace kccot
