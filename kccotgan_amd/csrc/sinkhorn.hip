// Log-domain Sinkhorn solve and its exact reverse sweep (replaces gan_utils.py:138-165 and
// :87-121 of the reference, and what tf.GradientTape records through that unrolled loop).
//
// One workgroup per n x n problem; the problem never leaves the CU.  The loop is a chain of
// 2*nits dependent half-steps, each one pass over the n^2 cost entries plus one reduction per
// line, so it is latency-bound: no per-iteration launches, no host sync for the stop rule, and
// for n <= 128 the cost matrix lives in registers in BOTH orientations:
//
//   row layout:    thread (i = t / LPR, q = t % LPR) owns C[i][q*EPT + m], m < EPT
//   column layout: thread (j = t / LPR, q = t % LPR) owns C[q*EPT + m][j], m < EPT
//
// LPR (lanes per line) is 8 or 16, i.e. at most one 16-lane DPP row: the log-sum-exp of a line
// is EPT serial terms + log2(LPR) DPP steps (quad_perm, row_half_mirror, row_mirror -- register
// to register, no LDS crossbar); the duals u and v are exchanged through 2*n floats of LDS
// (ds_read_b128: a thread's EPT entries are contiguous) with ONE barrier per half-step.
//
// The iteration is the reference's (max-shifted LSE over ((-C + u) + v)/eps, u then v with the new
// u), carried in log2 units so that exp/log are the hardware v_exp_f32 / v_log_f32 (see half_step).
#include "common.h"
#include <math.h>
#include "options.h"

// No floating-point contraction in this file: the solver kernels exist in several forms (forward / sweep / fused,
// different lanes per line) that are tested for BIT-identical results, and a mul + add that the compiler fuses into
// an fma in one form but not in another (it did, in the far regime, once the sweep's exp2 were hoisted) breaks that.
// The reference's TensorFlow ops do not fuse either.
#pragma clang fp contract(off)

namespace kccot {

constexpr int SK_MAXN = 128;      // register-resident kernels
constexpr int SK_FUSED_MAXPROB = 4;  // problems of one fused solve + sweep launch (sinkhorn_fused_reg)
constexpr int SK_MAXT = 1024;
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(x * LOG2E); }
__device__ __forceinline__ float fast_log(float x) { return __builtin_amdgcn_logf(x) * LN2; }

// Diagnostic build only (-DKCCOT_DIAG, libkccot_diag.so, tools/diag_sinkhorn.py): in-kernel
// s_memtime stamps of one half-step.  The product library contains no stamp.  The buffer is [problem, 16 waves,
// KCCOT_DIAG_SLOTS]; the slots of the fused kernels are listed in tools/diag_sinkhorn.py.
#ifdef KCCOT_DIAG
#ifndef KCCOT_DIAG_IT
#define KCCOT_DIAG_IT 50
#endif
#define KCCOT_DIAG_SLOTS 32
#define KCCOT_STAMP(SLOT) KCCOT_STAMP_IF(it == KCCOT_DIAG_IT, SLOT)
#define KCCOT_STAMP_IF(COND, SLOT)                                                                \
    do {                                                                                          \
        if (a.diag && (COND)) {                                                                   \
            unsigned long long tt_;                                                               \
            __builtin_amdgcn_sched_barrier(0);                                                    \
            asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tt_)::"memory");          \
            __builtin_amdgcn_sched_barrier(0);                                                    \
            if ((threadIdx.x & 63) == 0) a.diag[(blockIdx.x * 16 + (threadIdx.x >> 6)) * KCCOT_DIAG_SLOTS + (SLOT)] = tt_; \
        }                                                                                         \
    } while (0)
// the kernel's last stamp: taken once the wave's own stores and loads have completed
#define KCCOT_STAMP_DRAINED(SLOT)                                                                 \
    do {                                                                                          \
        if (a.diag) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                              \
        KCCOT_STAMP_IF(true, SLOT);                                                               \
    } while (0)
#else
#define KCCOT_STAMP(SLOT) do {} while (0)
#define KCCOT_STAMP_IF(COND, SLOT) do {} while (0)
#define KCCOT_STAMP_DRAINED(SLOT) do {} while (0)
#endif

struct SinkArgs {
    const float* C;       // [nprob,n,n]
    int n, L, Lmin, stop_mode;
    float eps, inv_eps, thresh;
    float* u_hist;        // [nprob,L,n] or null
    float* v_hist;
    float* cost_out;      // [nprob]
    int32_t* nits_out;    // [nprob]
    float* pi_out;        // [nprob,n,n] or null
    unsigned long long* diag;   // diagnostic build only; null otherwise
    float* loss_out;      // mixed divergence 2*cost[0]-cost[1]-cost[2] (nprob == 3), or null
    int* ticket;          // arrival counter for loss_out: zero on entry, reset to zero by the last workgroup
    int shortcut;         // 1: exact periodic-state shortcut enabled (shortcut_mismatch)
    // weighted marginals (the _w kernels only; an extension, not reference behaviour): strictly positive finite weights,
    // log taken once per lane before the loop.  w_div = 0: wa, wb are [nprob,n], problem p reads row p.  w_div = 1: wa =
    // w_real [n], wb = w_fake [n] and the three problems of the divergence read (a,b), (a,a), (b,b).  NULL: mu = nu = 1/n.
    // w_div = 2 (conditional mode, include/kccot_conditional.h): C is ONE shared C3 [3,n,n], wa = wb = w [Q,n]; problem
    // p = 3 q + k reads cost matrix k and weight row q for both marginals, everything else stays indexed by p.
    const float* wa;
    const float* wb;
    int w_div;
};

// the marginal weights of problem p (see SinkArgs::wa)
__device__ __forceinline__ const float* weights_of(const float* wa, const float* wb, int w_div, int p, int n, bool rows) {
    if (w_div == 2) return wa + (int64_t)(p / 3) * n;
    if (w_div) return rows ? (p == 2 ? wb : wa) : (p == 1 ? wa : wb);
    return (rows ? wa : wb) + (int64_t)p * n;
}
// a weight the solvers accept: strictly positive and finite (NaN fails the first comparison)
__device__ __forceinline__ bool weight_ok(float w) { return w > 0.f && w < INFINITY; }

// Load the EPT contiguous duals a thread needs (entries q*EPT .. q*EPT+EPT-1) from LDS.
template <int EPT>
__device__ __forceinline__ void load_other(float (&o)[EPT], const float* arr, int q) {
    if constexpr (EPT >= 4) {
#pragma unroll
        for (int m = 0; m < EPT; m += 4) {
            const float4 v = *reinterpret_cast<const float4*>(arr + q * EPT + m);
            o[m] = v.x; o[m + 1] = v.y; o[m + 2] = v.z; o[m + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int m = 0; m < EPT; ++m) o[m] = arr[q * EPT + m];
    }
}

typedef float f32x2 __attribute__((ext_vector_type(2)));

// Pins r[] in VGPRs at this point of the instruction stream.  lds_barrier() is an asm volatile with a memory clobber: that
// holds LDS and global accesses on their side of the barrier, but NOT register arithmetic, which the compiler is free to sink
// behind it (it did: the column role's whole plan of sinkhorn_fused_roles, 8 v_exp_f32 and their adds, went to the head of the
// chain pass that the role split exists to keep clear).  An empty asm volatile that takes the values as in/out operands emits
// no instruction; the values have to exist when it is reached, and asm volatile statements keep their order, so
// keep_in_regs(r); lds_barrier(); puts everything r[] depends on in front of the barrier.  The values are pinned as two-wide
// vectors (one aligned VGPR pair per operand), so that the v_pk_*_f32 that consume them keep their register pairs.
template <int N>
__device__ __forceinline__ void keep_in_regs(float (&r)[N]) {
    if constexpr (N >= 2) {
#pragma unroll
        for (int m = 0; m < N; m += 2) {
            f32x2 t = {r[m], r[m + 1]};
            asm volatile("" : "+v"(t));
            r[m] = t.x; r[m + 1] = t.y;
        }
    } else {
        asm volatile("" : "+v"(r[0]));
    }
}

// ---- log2-domain half-step ---------------------------------------------------------------------
// With k2 = log2(e)/eps the kernels carry  c2 = C*k2,  U = u*k2,  V = v*k2  and evaluate
//     y = (U_i - c2_ij) + V_j            [= ((-C+u)+v)/eps * log2(e), same association as gan_utils.py:153]
//     lse2 = log2(sum_j exp2(y - max)) + max,      U_i <- (log2(1/n) - lse2) + U_i
// which is the reference's update  u <- eps*(log(1/n) - LSE) + u  multiplied through by k2: two
// adds per entry instead of add/add/mul/mul, exp2/log2 are single hardware instructions, and the
// two-wide vector type lets hipcc issue packed v_pk_add_f32.  The iterates are the same numbers in
// other units; only fp32 rounding differs (the duals are O(1e3) with an ulp of 1e-4 either way).
// Trims of the forward half-step (profiles/sinkhorn_forward_trim_ab.json), a bit mask for experiment builds:
// in the role kernel 1 the DPP max as one asm statement (in the one-role kernel it measured +2 us: not there), and in the
// role kernel's instances without the shortcut
// 2 |du| formed off the chain and only when the stop rule reads it, 4 running row addresses, 16 the add tree on two-wide pairs;
// 32 (experiment, not in the product) |du| of sinkhorn_fused_reg and sinkhorn_fwd_body only when the stop rule reads it.
// (8 was the row role's self - c2 formed off the chain: measured slower, source not kept.)
#ifndef KCCOT_FWD_TRIM
#define KCCOT_FWD_TRIM 23
#endif

// The DPP max of a line's lanes as ONE asm statement.  common.h's seg_max is one statement per step, and behind every
// statement whose result the next instruction reads hipcc pads a wait state of its own (it cannot see what the statement
// wrote with): three s_nop 0 on the chain of the half-step at eight lanes per line.  As one statement the steps keep the
// s_nop 1 the DPP read of a fresh VALU result needs, and one pad is left, behind the last.  Same instructions on the same
// operands, same bits.
#define KCCOT_DPP_MAX_STEP(CTRL) "s_nop 1\n\tv_max_f32_dpp %0, %0, %0 " CTRL " row_mask:0xf bank_mask:0xf\n\t"
template <int LPR>
__device__ __forceinline__ float seg_max_chain(float v) {
    if constexpr (LPR >= 16)
        asm volatile(KCCOT_DPP_MAX_STEP("quad_perm:[1,0,3,2]") KCCOT_DPP_MAX_STEP("quad_perm:[2,3,0,1]")
                     KCCOT_DPP_MAX_STEP("row_half_mirror") KCCOT_DPP_MAX_STEP("row_mirror") : "+v"(v));
    else if constexpr (LPR >= 8)
        asm volatile(KCCOT_DPP_MAX_STEP("quad_perm:[1,0,3,2]") KCCOT_DPP_MAX_STEP("quad_perm:[2,3,0,1]")
                     KCCOT_DPP_MAX_STEP("row_half_mirror") : "+v"(v));
    else if constexpr (LPR >= 4)
        asm volatile(KCCOT_DPP_MAX_STEP("quad_perm:[1,0,3,2]") KCCOT_DPP_MAX_STEP("quad_perm:[2,3,0,1]") : "+v"(v));
    else if constexpr (LPR >= 2)
        asm volatile(KCCOT_DPP_MAX_STEP("quad_perm:[1,0,3,2]") : "+v"(v));
    return v;
}

// The LDS address of a word of a __shared__ array, and back: a 32-bit value that a loop can carry, move on and pin in a VGPR
// (keep_in_regs) where a pointer expression would be formed again from the loop counter in front of every access.
typedef __attribute__((address_space(3))) float lds_float;
__device__ __forceinline__ unsigned lds_address(const float* p) { return (unsigned)(size_t)(const lds_float*)p; }
__device__ __forceinline__ float* lds_pointer(unsigned a) { return (float*)(lds_float*)(size_t)a; }

// no stamp: the half-step of every product kernel (the diagnostic twin of the role kernel passes its own, see fused_roles_body)
struct NoStamp { __device__ __forceinline__ void operator()(int) const {} };

// The half-step behind its entries y[] = (U_i - c2_ij) + V_j: max, shifted exp2, sum, log2, new dual.  stamp(0) is called once
// the line's max is known, stamp(1) once its sum is (half_step calls stamp(-1) once the duals have arrived).
template <int EPT, int LPR, bool PAIRS = false, bool ONE_MAX = false, typename STAMP = NoStamp>
__device__ __forceinline__ float half_step_lse(const float (&y)[EPT], float self, float lw2, STAMP stamp = STAMP()) {
    float mx = y[0];
#pragma unroll
    for (int m = 1; m < EPT; ++m) mx = fmaxf(mx, y[m]);
    mx = ONE_MAX ? seg_max_chain<LPR>(mx) : seg_max<LPR>(mx);
    // tf.reduce_logsumexp: a non-finite max is replaced by 0
    const float shift = (mx > -INFINITY && mx < INFINITY) ? mx : 0.f;
    stamp(0);
    float e[EPT];
    if constexpr (EPT >= 2) {
        const f32x2 sh = {shift, shift};
#pragma unroll
        for (int m = 0; m < EPT; m += 2) {
            const f32x2 yy = {y[m], y[m + 1]};
            const f32x2 d = yy - sh;
            e[m] = __builtin_amdgcn_exp2f(d.x);
            e[m + 1] = __builtin_amdgcn_exp2f(d.y);
        }
    } else {
        e[0] = __builtin_amdgcn_exp2f(y[0] - shift);
    }
    // pairwise tree: log2(EPT) dependent adds instead of EPT
    if constexpr (PAIRS && EPT >= 4) {
        // The same tree with its two halves side by side: below its last level the tree adds within e[0 .. EPT/2) and within
        // e[EPT/2 .. EPT) by one pattern, so the pairs {e[k], e[k + EPT/2]} go through it as two-wide adds (v_pk_add_f32) and
        // the last level adds the two lanes of pair 0.  Same operands in every add, same bits.  hipcc finds this form by itself
        // in the callers that index the history rows by the loop counter and loses it with the running offsets of the role
        // kernel, which therefore asks for it (PAIRS); every other caller keeps the loop below.
        constexpr int H = EPT / 2;
        f32x2 pe[H];
#pragma unroll
        for (int k = 0; k < H; ++k) pe[k] = f32x2{e[k], e[k + H]};
#pragma unroll
        for (int w = 1; w < H; w *= 2)
#pragma unroll
            for (int m = 0; m + w < H; m += 2 * w) pe[m] += pe[m + w];
        e[0] = pe[0].x + pe[0].y;
    } else {
#pragma unroll
        for (int w = 1; w < EPT; w *= 2)
#pragma unroll
            for (int m = 0; m + w < EPT; m += 2 * w) e[m] += e[m + w];
    }
    const float s = seg_sum<LPR>(e[0]);
    stamp(1);
    const float lse2 = __builtin_amdgcn_logf(s) + shift;
    return (lw2 - lse2) + self;   // gan_utils.py:154,156 in log2 units
}

template <int EPT, int LPR, bool ROW, bool PAIRS = false, bool ONE_MAX = false, typename STAMP = NoStamp>
__device__ __forceinline__ float half_step(const float (&c2)[EPT], float self, const float* other, int q, float lw2,
                                           STAMP stamp = STAMP()) {
    float o[EPT];
    load_other<EPT>(o, other, q);
    stamp(-1);                                                 // the other role's duals have arrived
    float y[EPT];
    if constexpr (EPT >= 2) {
#pragma unroll
        for (int m = 0; m < EPT; m += 2) {
            f32x2 cc = {c2[m], c2[m + 1]}, oo = {o[m], o[m + 1]}, ss = {self, self};
            const f32x2 t = ROW ? ((ss - cc) + oo) : ((oo - cc) + ss);
            y[m] = t.x; y[m + 1] = t.y;
        }
    } else {
        y[0] = ROW ? ((self - c2[0]) + o[0]) : ((o[0] - c2[0]) + self);
    }
    return half_step_lse<EPT, LPR, PAIRS, ONE_MAX>(y, self, lw2, stamp);
}

// c2 = C * k2 in both orientations; entries past the matrix edge are +inf (-> exp2(-inf) = 0)
template <int EPT, int LPR>
__device__ __forceinline__ void load_costs(const float* __restrict__ C, int n, int line, int q, float k2,
                                           float (&crow)[EPT], float (&ccol)[EPT]) {
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        const int idx = q * EPT + m;
        const bool ok = line < n && idx < n;
        crow[m] = ok ? C[(int64_t)line * n + idx] * k2 : INFINITY;
        ccol[m] = ok ? C[(int64_t)idx * n + line] * k2 : INFINITY;
    }
}

// ---- stages shared by the register forms ---------------------------------------------------------
// sinkhorn_fwd_body, sinkhorn_bwd_body, sinkhorn_fused_reg and fused_roles_body are tested for BIT-identical results against
// each other; the stages that more than one of them runs are defined once, here.  Barriers, pins and stamps stay at the call
// sites, so that every wave of every form meets the same ones.  A stage is shared only where every kernel that calls it
// keeps its registers, scratch, LDS and the opcode sequence of every loop that holds a barrier; the fused LDS prologue, the
// forward's cost loop and ring fill and the sweep kernel's final-cost adjoint and dC write-back did not, and stay in their
// bodies.

// EXACT periodic-state shortcut.  One iteration is a deterministic function of the state (u,v).  As soon as the state after
// iteration k equals, bit for bit, the state after iteration k-p (p <= 4) the sequence is periodic from there on, and the
// state after any later iteration K is a stored state congruent to K modulo p: nothing is approximated, the loop is merely
// not re-executed.  (Sharp problems -- costs of O(1e3) against eps = 1, the GAN regime -- reach an fp32 fixed point within a
// handful of iterations.)  The kernel jumps to one iteration before the first point at which the reference's stop rule
// could fire (or before L), fills the history the backward needs, and resumes the ordinary loop, so the stop logic and the
// final iterate are computed by the same code as without the shortcut.  nits_out[p] is the reference-equivalent iteration
// count; nits_out[nprob + p] the number of iterations actually executed.
//
// Detection costs no LDS round trip on the critical path: every lane keeps its line's last four duals in registers and
// compares in place (shortcut_mismatch); one ballot per candidate period folds the wave's lines, lane 0 ORs the wave's mismatch
// mask into an LDS word (shortcut_vote), and the word is read back after the closing barrier but only CONSUMED one
// iteration later (shortcut_period: its latency hides under the next half-step).
//
// step (a): ORs into `bits` bit pp <=> the new dual sn differs from the one pp iterations earlier (cur: one iteration
// earlier, p2 .. p4: the line's ring).  The ring stays three plain floats of the caller, which moves it on by one
// (p4 = p3; p3 = p2; p2 = cur) right after the call: taken by reference the ring is promoted to registers only after
// inlining, and the forward loops of the one-role kernels came out scheduled differently.
__device__ __forceinline__ void shortcut_mismatch(int& bits, float sn, float cur, float p2, float p3, float p4) {
    const unsigned b = __float_as_uint(sn);
    bits |= (b != __float_as_uint(cur) ? 2 : 0) | (b != __float_as_uint(p2) ? 4 : 0) |
           (b != __float_as_uint(p3) ? 8 : 0) | (b != __float_as_uint(p4) ? 16 : 0);
}
// step (b): the wave's vote into mis[it & 3]
__device__ __forceinline__ void shortcut_vote(int bits, bool active, int t, int* mis, int it) {
    if (!active) bits = 0;
    int wb = 0;
#pragma unroll
    for (int pp = 1; pp <= 4; ++pp)
        if (__builtin_amdgcn_ballot_w64((bits >> pp) & 1)) wb |= 1 << pp;
    if ((t & 63) == 0 && wb) atomicOr(&mis[it & 3], wb);
}
// step (c), at the end of iteration `it`: the smallest period the PREVIOUS iteration's votes allow (0: none).  mprev
// describes iteration it-1: bit pp clear <=> S_it == S_{it-pp} (valid for it-1 >= pp).
__device__ __forceinline__ int shortcut_period(int* mis, int it, int t, int& mprev) {
    const int mcur = mis[it & 3];                 // consumed at the end of the NEXT iteration
    if (t == 0) mis[(it + 2) & 3] = 0;
    int per = 0;
#pragma unroll
    for (int pp = 4; pp >= 1; --pp)
        if (it - 1 >= pp && !((mprev >> pp) & 1)) per = pp;
    mprev = mcur;
    return per;
}
// ... and the iteration count K1 to resume at, so that iteration K1+1, the first at which the reference could leave its
// loop early (or the last one), is real
__device__ __forceinline__ int shortcut_resume(int L, int Lmin, int stop_mode) {
    int first_stop = (stop_mode == KCCOT_STOP_INDEX) ? Lmin + 1 : Lmin;
    if (first_stop < 1) first_stop = 1;
    return (L < first_stop ? L : first_stop) - 1;
}
// The history fill of the jump in the fused kernels, whose history is in LDS: the states from S_{nits-per+1} on repeat with
// period per, so row k <- row lo + (k - lo) mod per for k in (nits, K1].  (sinkhorn_fwd_body fills from its LDS ring instead.)
__device__ __forceinline__ void fill_history_rows(float* hu, float* hv, int NS, int n, int t, int nits, int K1, int per) {
    const int lo = nits - per + 1;
    for (int e = t; e < (K1 - nits) * n; e += blockDim.x) {
        const int k = nits + 1 + e / n, i = e % n;
        const int src = lo + (k - lo) % per;
        hu[k * NS + i] = hu[src * NS + i];
        hv[k * NS + i] = hv[src * NS + i];
    }
}

// gan_utils.py:162-164 in the fused kernels: pi = exp((-C + u + v^T)/eps); cost = sum(pi * C) over a row-layout lane's
// entries.  craw[] holds the lane's elements of C as the prologue loaded them (load_costs_raw): no global access stands
// between the two loops.  sinkhorn_fwd_body keeps its own loop, which also writes and poisons the plan.
template <int EPT>
__device__ __forceinline__ float cost_partial(const float (&crow)[EPT], const float (&craw)[EPT], float ui, const float* v,
                                              int n, int q, bool active) {
    // no branch per entry: the duals arrive in one vector read (pad columns of a history row are zero) and an entry past the
    // edge is skipped by a select, which leaves the sum of the others, in their order, as it was
    float ov[EPT];
    load_other<EPT>(ov, v, q);
    float part = 0.f;
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        const float pi = __builtin_amdgcn_exp2f((ui - crow[m]) + ov[m]);
        const float sum = part + pi * craw[m];
        part = (active && q * EPT + m < n) ? sum : part;
    }
    return part;
}
// one orientation of load_costs that also keeps the elements themselves (0 past the edge) for cost_partial
template <int EPT, bool ROW>
__device__ __forceinline__ void load_costs_raw(const float* C, int n, int line, int q, float k2, float (&c2)[EPT],
                                               float (&craw)[EPT]) {
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        const int idx = q * EPT + m;
        const bool ok = line < n && idx < n;
        craw[m] = ok ? C[ROW ? (int64_t)line * n + idx : (int64_t)idx * n + line] : 0.f;
        c2[m] = ok ? craw[m] * k2 : INFINITY;
    }
}
template <int EPT, bool ROW>
__device__ __forceinline__ void load_costs_raw(const float* C, int n, int line, int q, float k2, float (&c2)[EPT]) {
    float craw[EPT];
    load_costs_raw<EPT, ROW>(C, n, line, q, k2, c2, craw);
}

// A NaN cost or NaN entry of dC leaves the register kernels for n <= 64 (fused bodies, sinkhorn_fwd_body, sinkhorn_bwd_body below
// 16 entries per lane) as the quiet NaN 0x7fc00000.  A change of behaviour on non-finite inputs: before, the sign of such a NaN
// was whatever the kernel's arithmetic left.  NOT covered: the dual histories, the plan, the sweep kernels at 16 entries per lane
// (n > 64: sinkhorn_bwd_body there is at its register cap, and the select moved its sweep loop and its spills), the multi-CU and
// streaming kernels.  Which operand's NaN an add or a
// multiply hands on follows the operand order hipcc picks for a commutative operation, per kernel and per build, so the sign of
// a NaN result differed between the fused and the two-launch forms and moved with unrelated changes of a loop
// (tests/test_gpu_forward_trim.py, non-finite cost matrices).  One compare and one select per stored word, behind the loops.
__device__ __forceinline__ float canonical_nan(float x) { return x != x ? __uint_as_float(0x7fc00000u) : x; }

// The cost of a fused problem, by the one thread that hands it off: the waves' partial sums (wave_sum of cost_partial, parked
// in red[] in front of the barrier of the dC transpose) added in wave order to + 0.0f, as block_sum adds them.
// All 16 words are read at once (a loop over nw is one LDS round trip per wave, on the thread the kernel's end waits for);
// the words of waves that do not exist are skipped by a select.
__device__ __forceinline__ float cost_of_waves(const float* red, int nw) {
    float v[16];
#pragma unroll
    for (int w = 0; w < 16; ++w) v[w] = red[w];
    float r = 0.f;
#pragma unroll
    for (int w = 0; w < 16; ++w) r = w < nw ? r + v[w] : r;
    return r;
}

// Thread 0 of problem p publishes its cost and iteration counts; with `combine`, the last of the NPROB workgroups to arrive
// writes loss = sum_p w[p] cost[p], added left to right: (2 c0 - c1) - c2 on three problems (gan_utils.py:225),
// ((c0 + c1) - c2) - c3 on four (w[p] = +-1 or 2, so w[p] c[p] is exact and x + (-c) == x - c).
// Placement-independent hand-off without fences -- the FIRST ROW of MI355X_MICROARCH.md's table of measured hand-offs ("one
// lane of each storing workgroup ... an agent-scope atomic add; the workgroup whose add came last, told by the value its add
// returned, loads only after its add has returned; stores all sc1, loads all sc1, 4-byte"): the handed-off word is stored
// with agent scope (written through), the store drained (vmcnt(0)), then the relaxed ticket; the last arriver reads the
// costs with agent-scope loads.  This is gfx950 behaviour, not a guarantee of the HIP memory model (under which it is a
// race): the emitted cache-policy bits and the drain are pinned by
// tests/test_abi.py::test_isa_of_the_three_cost_hand_off_to_the_combining_workgroup, and this library builds for gfx950
// only.  (Until round 3: plain store + agent release fence + acquire fence in the last arriver -- an L2 write-back and an L1
// invalidate, ~1.7 us each, on the one thread the workgroup then waits for.)
// Three words are read back either way: on four problems the combining workgroup's own cost is the one in its register.
// The pointers are taken as references to the members of the kernel-argument struct ON PURPOSE: by value all four are loaded
// at the call, ahead of the branches that use them, and the one-role fused kernels came out with two more SGPRs.
template <int NPROB>
__device__ __forceinline__ void publish_cost(float* const& cost_out, int32_t* const& nits_out, float* const& loss_out,
                                             int* const& ticket, int p, float cost, int nits, int computed, const float* w,
                                             bool combine) {
    __hip_atomic_store(cost_out + p, cost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    nits_out[p] = nits;
    nits_out[gridDim.x + p] = computed;
    if (!combine) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tk == (int)gridDim.x - 1) {
        float c[NPROB];
        if constexpr (NPROB == 3) {
#pragma unroll
            for (int pp = 0; pp < 3; ++pp) c[pp] = __hip_atomic_load(cost_out + pp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            float o[3];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                o[k] = __hip_atomic_load(cost_out + ((p + 1 + k) & 3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int pp = 0; pp < 4; ++pp) {
                const int k = (pp - p - 1) & 3;                    // pp = (p + 1 + k) & 3; k = 3 is p itself
                c[pp] = k == 0 ? o[0] : k == 1 ? o[1] : k == 2 ? o[2] : cost;
            }
        }
        float l = w[0] * c[0];
#pragma unroll
        for (int pp = 1; pp < NPROB; ++pp) l += w[pp] * c[pp];
        loss_out[0] = l;
        __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Adjoint of the final cost, one entry of one orientation.  cost = sum_ij pi_ij C_ij, pi = exp2((U - c2) + V);  C/eps = c2*ln2:
//   dcost/dC_ij (direct) = pi_ij (1 - C_ij/eps); dcost/du_i = sum_j pi_ij C_ij/eps; same for v
// ROW: d = g * (direct term) and ss += pi_ij c2_ij, the line's part of dcost/du_i; column: d = 0 and the part of dcost/dv_j.
// The loop over a lane's entries and the seg_sum stay with the caller: sinkhorn_fused_reg takes both orientations of an
// entry in one loop trip, a role takes its own (sinkhorn_bwd_body keeps its own block).  gu[line] / gv[line] = g * seg_sum(ss) * LN2.
template <bool ROW>
__device__ __forceinline__ void final_cost_adjoint(float c2, float self, float other, bool ok, float g, float& d, float& ss) {
    const float cc = ok ? c2 : 0.f;
    const float pv = ok ? __builtin_amdgcn_exp2f(ROW ? ((self - cc) + other) : ((other - cc) + self)) : 0.f;
    d = ROW ? g * pv * (1.f - cc * LN2) : 0.f;
    ss += pv * cc;
}

// dC = row-layout part + (column-layout part)^T in the fused kernels.  The transpose goes through LDS: the column lanes park
// their entries in an n x n tile at pitch n + 1 (park_dc_cols), the caller's lds_barrier() follows, the row lanes add the
// transposed entries to their own (take_dc_cols; x + y has the same bits whichever side adds) and store every row once
// (store_dc_rows).  The tile lies on the dual history, which is dead by then: every wave is behind the sweep's last barrier
// (with no iteration at all, behind the barrier that follows the last read of row 0); the host sizes the dynamic LDS for the
// larger of the two (fused_lds_bytes).  Pad lines and pad columns are neither written nor read.
template <int EPT>
__device__ __forceinline__ void park_dc_cols(float* tile, const float (&dcol)[EPT], int n, int line, int q, bool active) {
    if (active) {
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const int idx = q * EPT + m;
            if (idx < n) tile[idx * (n + 1) + line] = dcol[m];
        }
    }
}
template <int EPT>
__device__ __forceinline__ void take_dc_cols(const float* tile, float (&drow)[EPT], int n, int line, int q, bool active) {
    // every read is issued before the first is waited for: an entry past the edge reads word 0 of the tile instead (its sum is
    // never stored)
#pragma unroll
    for (int m = 0; m < EPT; ++m) {
        const int idx = q * EPT + m;
        drow[m] += tile[(active && idx < n) ? line * (n + 1) + idx : 0];
    }
}
template <int EPT>
__device__ __forceinline__ void store_dc_rows(float* dC, const float (&drow)[EPT], int n, int line, int q, bool active) {
    if (active) {
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const int idx = q * EPT + m;
            if (idx < n) dC[(int64_t)line * n + idx] = canonical_nan(drow[m]);
        }
    }
}

template <int EPT, int LPR, bool SHORTCUT, bool WEIGHTED>
__device__ __forceinline__ void sinkhorn_fwd_body(const SinkArgs& a) {
    // padded so that the float4 reads of lines past n stay inside the arrays
    __shared__ __attribute__((aligned(16))) float u_s[SK_MAXN + 16 * 16];
    __shared__ __attribute__((aligned(16))) float v_s[SK_MAXN + 16 * 16];
    __shared__ float red[16];
    const int p = blockIdx.x, n = a.n;
    const int t = threadIdx.x, line = t / LPR, q = t % LPR;
    const bool active = line < n;
    int pc = p;          // the cost matrix this problem reads: its own, or (conditional mode) matrix p % 3 of the shared C3
    if constexpr (WEIGHTED) { if (a.w_div == 2) pc = p % 3; }
    const float* C = a.C + (int64_t)pc * n * n;
    const float k2 = a.inv_eps * LOG2E;

    float crow[EPT], ccol[EPT];
    load_costs<EPT, LPR>(C, n, line, q, k2, crow, ccol);
    for (int i = t; i < SK_MAXN + 16 * 16; i += blockDim.x) { u_s[i] = 0.f; v_s[i] = 0.f; }   // gan_utils.py:147
    __syncthreads();

    const float lw2 = __builtin_amdgcn_logf(1.0f / (float)n);   // log2(mu) = log2(nu), gan_utils.py:138-139
    // log2 of this line's marginals: the constant, or (WEIGHTED) the line's own weights, loaded and checked ONCE here.  A
    // weight that is <= 0 or not finite poisons the whole problem (NaN cost, nits = -1: the convention of an aborted
    // multi-CU solve) instead of producing a finite, plausible and wrong cost; the loop is then not entered.
    float lwu = lw2, lwv = lw2;
    bool bad = false;
    if constexpr (WEIGHTED) {
        const float wu = active ? weights_of(a.wa, a.wb, a.w_div, p, n, true)[line] : 1.f;
        const float wv = active ? weights_of(a.wa, a.wb, a.w_div, p, n, false)[line] : 1.f;
        bad = __syncthreads_or(!(weight_ok(wu) && weight_ok(wv)));
        lwu = __builtin_amdgcn_logf(wu);
        lwv = __builtin_amdgcn_logf(wv);
    }
    const int Lrun = (WEIGHTED && bad) ? 0 : a.L;
    // stop rule in log2 units: sum|u-u_prev| = sum|U-U_prev| * eps*ln2
    const float err_scale = a.eps * LN2;

    // The exact periodic-state shortcut (shortcut_mismatch).  The ring of the last four states in LDS is written every iteration and
    // read only at the jump.
    __shared__ float ring_u[4][SK_MAXN], ring_v[4][SK_MAXN];
    __shared__ int mis[4];
    if (SHORTCUT) {
        if (t < 4) mis[t] = 0;
        __syncthreads();
    }
    bool detect = SHORTCUT;
    int computed = 0;
    int mprev = ~0;                       // mismatch mask of the previous iteration (bit p: state != state p iterations earlier)
    float pu2 = 0.f, pu3 = 0.f, pu4 = 0.f, pv2 = 0.f, pv3 = 0.f, pv4 = 0.f;

    int nits = 0;
    float ui = 0.f, vj = 0.f;   // this line's duals (every lane of the line holds them)
    for (int it = 0; it < Lrun; ++it) {
        // every lane executes the half-steps (DPP reads neighbours); only real lines store
        KCCOT_STAMP(0);
        const float un = half_step<EPT, LPR, true>(crow, ui, v_s, q, lwu);
        KCCOT_STAMP(1);
        float du = 0.f;
        if (!(KCCOT_FWD_TRIM & 32) || (((a.stop_mode == KCCOT_STOP_INDEX) ? it >= a.Lmin : it + 1 >= a.Lmin) && it + 1 < a.L)) du = (active && q == 0) ? fabsf(un - ui) : 0.f;
        int bits = 0;
        if (SHORTCUT && detect) {
            shortcut_mismatch(bits, un, ui, pu2, pu3, pu4);
            pu4 = pu3; pu3 = pu2; pu2 = ui;
        }
        ui = un;
        if (active && q == 0) {
            u_s[line] = un;
            if (a.u_hist) a.u_hist[((int64_t)p * a.L + it) * n + line] = un;
            if (SHORTCUT && detect) ring_u[it & 3][line] = un;
        }
        KCCOT_STAMP(2);
        lds_barrier();      // the history stores stay in flight (nothing in this kernel reads them back)
        KCCOT_STAMP(3);
        const float vn = half_step<EPT, LPR, false>(ccol, vj, u_s, q, lwv);
        KCCOT_STAMP(4);
        if (SHORTCUT && detect) {
            shortcut_mismatch(bits, vn, vj, pv2, pv3, pv4);
            pv4 = pv3; pv3 = pv2; pv2 = vj;
            shortcut_vote(bits, active, t, mis, it);
        }
        vj = vn;
        if (active && q == 0) {
            v_s[line] = vn;
            if (a.v_hist) a.v_hist[((int64_t)p * a.L + it) * n + line] = vn;
            if (SHORTCUT && detect) ring_v[it & 3][line] = vn;
        }
        KCCOT_STAMP(5);
        lds_barrier();
        KCCOT_STAMP(6);
        nits = it + 1;
        ++computed;
        // gan_utils.py:157-160 (count-based) / :115-117 (index-based).  err is only needed once
        // the stop rule can fire, and never on the last iteration.
        const bool reached = (a.stop_mode == KCCOT_STOP_INDEX) ? (it >= a.Lmin) : (nits >= a.Lmin);
        if (reached && it + 1 < a.L) {
            const float err = block_sum(du, red) * err_scale;
            if (a.thresh > err) break;
        }
        if (SHORTCUT && detect) {
            const int per = shortcut_period(mis, it, t, mprev);
            KCCOT_STAMP(7);
            if (per) {
                detect = false;
                const int K1 = shortcut_resume(a.L, a.Lmin, a.stop_mode);
                if (K1 > nits) {
                    // the states from S_{it-per} on have period per, and the ring holds S_{nits-3..nits}
                    // (S_k in slot (k-1) & 3): S_k = S_src(k), src(k) = lo + (k - lo) mod per, lo = nits-per+1
                    const int lo = nits - per + 1;
                    if (a.u_hist) {
                        for (int e = t; e < (K1 - nits) * n; e += blockDim.x) {
                            const int k = nits + 1 + e / n, i = e % n;
                            const int slot = (lo + (k - lo) % per - 1) & 3;
                            a.u_hist[((int64_t)p * a.L + (k - 1)) * n + i] = ring_u[slot][i];
                            a.v_hist[((int64_t)p * a.L + (k - 1)) * n + i] = ring_v[slot][i];
                        }
                    }
                    const int slot = (lo + (K1 - lo) % per - 1) & 3;
                    if (t < n) { u_s[t] = ring_u[slot][t]; v_s[t] = ring_v[slot][t]; }
                    __syncthreads();
                    ui = u_s[active ? line : 0];
                    vj = v_s[active ? line : 0];
                    nits = K1;
                    it = K1 - 1;
                }
            }
        }
    }

    // gan_utils.py:162-164: pi = exp((-C + u + v^T)/eps); cost = sum(pi * C)   (C re-read: L2-resident)
    float part = 0.f;
    if (active) {
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const int idx = q * EPT + m;
            if (idx < n) {
                float pi = __builtin_amdgcn_exp2f((ui - crow[m]) + v_s[idx]);
                if (WEIGHTED && bad) pi = NAN;
                part += pi * C[(int64_t)line * n + idx];
                if (a.pi_out) a.pi_out[(int64_t)p * n * n + (int64_t)line * n + idx] = pi;
            }
        }
    }
    float cost = block_sum(part, red);
    if (WEIGHTED && bad) { cost = NAN; nits = -1; }
    if (t == 0) {
        // with loss_out, the last of the three workgroups to arrive combines the costs (gan_utils.py:225)
        const float w[3] = {2.0f, -1.0f, -1.0f};
        publish_cost<3>(a.cost_out, a.nits_out, a.loss_out, a.ticket, p, canonical_nan(cost), nits, computed, w, a.loss_out != nullptr);
    }
}

// the default (exact periodic-state shortcut compiled in) and the every-iteration variant
template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_fwd_reg(SinkArgs a) { sinkhorn_fwd_body<EPT, LPR, true, false>(a); }
template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_fwd_reg_full(SinkArgs a) { sinkhorn_fwd_body<EPT, LPR, false, false>(a); }
// the same two with weighted marginals (SinkArgs::wa / wb)
template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_fwd_reg_w(SinkArgs a) { sinkhorn_fwd_body<EPT, LPR, true, true>(a); }
template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_fwd_reg_full_w(SinkArgs a) { sinkhorn_fwd_body<EPT, LPR, false, true>(a); }

// ------------------------------------------------------------------------------------------
// reverse sweep
//   u_t,i = a - eps*LSE_j((-C_ij + u_{t-1,i} + v_{t-1,j})/eps) + u_{t-1,i},  a = eps*log(1/n)
//   v_t,j = a - eps*LSE_i((-C_ij + u_{t,i}   + v_{t-1,j})/eps) + v_{t-1,j}
// With P_t = softmax_j of the first argument and Q_t = softmax_i of the second:
//   du_t/dv_{t-1} = -P_t,  du_t/dC = +P_t,  du_t/du_{t-1} = 1 - sum_j P_t = 0
//   dv_t/du_t     = -Q_t,  dv_t/dC = +Q_t,  dv_t/dv_{t-1} = 1 - sum_i Q_t = 0
// and, from the update rules themselves, no reduction has to be redone:
//   Q_t[i,j] = exp((-C_ij + u_t,i + v_t,j     - a)/eps) = exp2((U_t,i - c2_ij) + V_t,j     - log2(1/n))
//   P_t[i,j] = exp((-C_ij + u_t,i + v_{t-1,j} - a)/eps) = exp2((U_t,i - c2_ij) + V_{t-1,j} - log2(1/n))
// (the two "= 0" terms are 1e-7-sized rounding residues in the reference's tape; dropped).
// The history holds the duals in the forward's log2 units (U, V); gradients are in natural units.
//
// Per iteration, newest first:   (A) row pass with Q_t:    gu_i -= sum_j Q_ij gv_j ; dC += Q_ij gv_j
//                                (B) column pass with P_t: gv_j = -sum_i P_ij gu_i ; dC += P_ij gu_i
// u_t / v_t come from the forward's history; the vectors of the NEXT (older) iteration are
// prefetched from global memory into registers one iteration ahead and parked in a
// double-buffered LDS slot, so the dependent chain sees LDS latency only: two barriers per
// iteration.
// ------------------------------------------------------------------------------------------
struct SinkBwdArgs {
    const float* C;
    const float* u_hist;
    const float* v_hist;
    const int32_t* nits;
    const float* gcost;   // [nprob], or with div_weights: ONE upstream scalar dLoss/dloss
    float* dC;
    int n, L;
    float eps, inv_eps;
    int div_weights;      // 1: gcost[p] = {2,-1,-1}[p] * gcost[0]   (d(2 xy - xx - yy), gan_utils.py:225)
    const float* wa;      // weighted marginals as in SinkArgs (sinkhorn_bwd_reg_w only); w_div = 2: C is the shared C3
    const float* wb;
    int w_div;
    float* da;            // [nprob,n] dcost/da, dcost/db scaled by gcost (the _dw kernels only; see sinkhorn_bwd_body)
    float* db;
};

// WEIGHTED (mu = a, nu = b): the column sums of the second argument are b_j and the row sums of the first a_i, so
//   Q_t[i,j] = exp2((U_t,i - c2_ij) + (V_t,j - log2 b_j)),   P_t[i,j] = exp2(((U_t,i - log2 a_i) - c2_ij) + V_{t-1,j})
// -- the one place where the sweep substitutes the marginal for a sum of a plan.  The shifted duals U - log2 a and
// V - log2 b are formed by the thread that refills the LDS slots (off the dependent chain) and parked beside the plain
// ones, so a pass costs the same instructions as with the constant; everything else is unchanged (log a and log b enter
// the updates additively; the weights themselves are not differentiated).  A problem the forward poisoned (nits < 0: a
// weight <= 0 or not finite) gets NaN gradients.
// DW (with WEIGHTED; include/kccot_weight_grad.h): the weights ARE differentiated.  u_t = eps log a + (terms without a direct
// a), v_t = eps log b + (...), so with gu_t the adjoint of u_t that gu[] holds after pass A of iteration t and gv_t the
// adjoint of v_t that gv[] holds when pass A of iteration t starts (gv_nits: the final-cost term)
//   dcost/da_i = (eps / a_i) sum_{t=1..nits} gu_t[i],      dcost/db_j = (eps / b_j) sum_{t=1..nits} gv_t[j]
// (what pass B writes at it == 1 is the adjoint of the constant v_0 = 0 and is not added).  The two running sums live in
// LDS beside gu / gv, in double, entry `line` touched only by the thread that writes gu[line] / gv[line]: one private
// read-add-write per line and half-step, no atomic, no barrier of its own, nothing on the dependent chain.  The factor
// eps / a_i is applied once, at the end.  dC is computed by the same instructions as without DW.
// The conserved mode.  Q_t has column sums 1 and P_t row sums 1, so sum_i gu_t[i] = -sum_j gv_t[j] and sum_j gv_{t-1}[j] =
// -sum_i gu_t[i]: the total of the adjoints is handed on unchanged from half-step to half-step, and it starts at
// sum_i gu_nits[i] = g cost/eps - g cost/eps = 0.  Exactly, every total is therefore zero (but that of gv_nits); in fp32 the
// first one is a rounding residue, it never decays (eigenvalue 1), and nits copies of it end up in the sums -- the one error
// of da / db that grows with the iteration count.  Its shape is known (a_i in gu, b_j in gv, the marginals of the plans), and
// so is its true amplitude (zero), so it is removed at the end: sa_i -= a_i sum(sa) / sum(a), likewise sb without the
// final-cost term, which is kept apart in gvf[].  One wave, once per launch, after the loop.
template <int EPT, int LPR, bool WEIGHTED, bool DW = false>
__device__ __forceinline__ void sinkhorn_bwd_body(const SinkBwdArgs& a) {
    static_assert(WEIGHTED || !DW, "the weight gradient belongs to the weighted sweep");
    constexpr int PADN = SK_MAXN + 16 * 16;
    __shared__ __attribute__((aligned(16))) float Ua[WEIGHTED ? 2 : 1][WEIGHTED ? PADN : 4];
    __shared__ __attribute__((aligned(16))) float Va[WEIGHTED ? 2 : 1][WEIGHTED ? PADN : 4];
    __shared__ float lab[WEIGHTED ? 2 : 1][WEIGHTED ? SK_MAXN : 1];     // log2 a, log2 b: entry t is thread t's alone
    __shared__ __attribute__((aligned(16))) float U[2][PADN];
    __shared__ __attribute__((aligned(16))) float V[2][PADN];
    __shared__ __attribute__((aligned(16))) float gu[PADN];
    __shared__ __attribute__((aligned(16))) float gv[PADN];
    __shared__ double sab[DW ? 2 : 1][DW ? SK_MAXN : 1];                // sum_t gu_t, sum_{t<nits} gv_t: entry `line` is its owner's alone
    __shared__ float gvf[DW ? SK_MAXN : 1];                             // gv_nits, the final-cost term
    __shared__ double mode[DW ? 2 : 1];                                 // amplitude of the conserved mode in sab[0], sab[1]
    const int p = blockIdx.x, n = a.n;
    const int t = threadIdx.x, line = t / LPR, q = t % LPR;
    const bool active = line < n;
    int pc = p;          // the cost matrix this problem reads: its own, or (conditional mode) matrix p % 3 of the shared C3
    if constexpr (WEIGHTED) { if (a.w_div == 2) pc = p % 3; }
    const float* C = a.C + (int64_t)pc * n * n;
    const float k2 = a.inv_eps * LOG2E;
    const float g = a.div_weights ? (p == 0 ? 2.0f : -1.0f) * a.gcost[0] : a.gcost[p];
    const int nits = a.nits[p];
    const float* uh = a.u_hist + (int64_t)p * a.L * n;
    const float* vh = a.v_hist + (int64_t)p * a.L * n;
    if constexpr (WEIGHTED) {
        if (nits < 0) {           // block-uniform
            if (active) {
#pragma unroll
                for (int m = 0; m < EPT; ++m) {
                    const int idx = q * EPT + m;
                    if (idx < n) a.dC[(int64_t)p * n * n + (int64_t)line * n + idx] = NAN;
                }
                if constexpr (DW) {
                    if (q == 0) { a.da[(int64_t)p * n + line] = NAN; a.db[(int64_t)p * n + line] = NAN; }
                }
            }
            return;
        }
        if (t < n) {    // kept in LDS, not in two registers: the EPT = 16 forms run at the 128-VGPR cap
            lab[0][t] = __builtin_amdgcn_logf(weights_of(a.wa, a.wb, a.w_div, p, n, true)[t]);
            lab[1][t] = __builtin_amdgcn_logf(weights_of(a.wa, a.wb, a.w_div, p, n, false)[t]);
        }
    }

    float crow[EPT], ccol[EPT], drow[EPT], dcol[EPT];
    load_costs<EPT, LPR>(C, n, line, q, k2, crow, ccol);
#pragma unroll
    for (int m = 0; m < EPT; ++m) { drow[m] = 0.f; dcol[m] = 0.f; }
    for (int i = t; i < PADN; i += blockDim.x) {
        U[0][i] = U[1][i] = V[0][i] = V[1][i] = 0.f;
        gu[i] = gv[i] = 0.f;
        if constexpr (WEIGHTED) Ua[0][i] = Ua[1][i] = Va[0][i] = Va[1][i] = 0.f;
    }
    if constexpr (DW) { if (t < SK_MAXN) sab[0][t] = sab[1][t] = 0.0; }
    __syncthreads();
    // history index k holds (U_{k+1}, V_{k+1}); iteration `it` (1-based) lives in slot it & 1;
    // V_0 = 0
    auto hist_u = [&](int it, int i) { return it >= 1 ? uh[(int64_t)(it - 1) * n + i] : 0.f; };
    auto hist_v = [&](int it, int i) { return it >= 1 ? vh[(int64_t)(it - 1) * n + i] : 0.f; };
    if (t < n) {
        U[nits & 1][t] = hist_u(nits, t);
        V[nits & 1][t] = hist_v(nits, t);
        V[(nits - 1) & 1][t] = hist_v(nits - 1, t);
        if constexpr (WEIGHTED) {
            Ua[nits & 1][t] = hist_u(nits, t) - lab[0][t];
            Va[nits & 1][t] = hist_v(nits, t) - lab[1][t];
            Va[(nits - 1) & 1][t] = hist_v(nits - 1, t) - lab[1][t];
        }
    }
    // prefetch for the first in-loop refill: U_{nits-1}, V_{nits-2}
    float nu = (t < n) ? hist_u(nits - 1, t) : 0.f;
    float nv = (t < n) ? hist_v(nits - 2, t) : 0.f;
    __syncthreads();

    const int lsafe = active ? line : 0;
    // cost = sum_ij pi_ij C_ij, pi = exp2((U - c2) + V);  C/eps = c2*ln2:
    //   dcost/dC_ij (direct) = pi_ij (1 - C_ij/eps); dcost/du_i = sum_j pi_ij C_ij/eps; same for v
    {
        const float* Uc = U[nits & 1];
        const float* Vc = V[nits & 1];
        const float ui = Uc[lsafe], vj = Vc[lsafe];
        float ov[EPT], ou[EPT];
        load_other<EPT>(ov, Vc, q);
        load_other<EPT>(ou, Uc, q);
        float su = 0.f, sv = 0.f;
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const bool ok = active && (q * EPT + m) < n;
            const float cr = ok ? crow[m] : 0.f, cc = ok ? ccol[m] : 0.f;
            const float pr = ok ? __builtin_amdgcn_exp2f((ui - cr) + ov[m]) : 0.f;
            drow[m] = g * pr * (1.f - cr * LN2);
            su += pr * cr;
            const float pc = ok ? __builtin_amdgcn_exp2f((ou[m] - cc) + vj) : 0.f;
            sv += pc * cc;
        }
        su = seg_sum<LPR>(su);
        sv = seg_sum<LPR>(sv);
        if (active && q == 0) {
            const float gvn = g * sv * LN2;
            gu[line] = g * su * LN2; gv[line] = gvn;
            if constexpr (DW) gvf[line] = nits > 0 ? gvn : 0.f;                  // with no iteration v = v_0, a constant
        }
    }
    const float lw2 = __builtin_amdgcn_logf(1.0f / (float)n);
    __syncthreads();

    for (int it = nits; it >= 1; --it) {
        const float* Uc = U[it & 1];
        const float* Vc = V[it & 1];
        const float* Vp = V[(it - 1) & 1];
        // (A) through v_t: row pass with Q_t
        {
            const float ui = WEIGHTED ? Uc[lsafe] : Uc[lsafe] - lw2;
            float ov[EPT], og[EPT];
            load_other<EPT>(ov, WEIGHTED ? Va[it & 1] : Vc, q);
            load_other<EPT>(og, gv, q);
            float s = 0.f;
#pragma unroll
            for (int m = 0; m < EPT; ++m) {
                // entries past the edge: c2 = +inf -> exp2(-inf) = 0
                const float w = __builtin_amdgcn_exp2f((ui - crow[m]) + ov[m]) * og[m];
                drow[m] += w;
                s += w;
            }
            s = seg_sum<LPR>(s);
            // grad wrt u_t: the final-cost term on the last iteration, nothing on older ones
            if (active && q == 0) {
                const float gun = (it == nits ? gu[line] : 0.f) - s;
                gu[line] = gun;
                if constexpr (DW) sab[0][line] += (double)gun;
            }
        }
        lds_barrier();      // LDS-only: the history prefetch (nu, nv) stays in flight across it
        // refill the slots the older iteration needs: U[(it-1)&1] <- U_{it-1}, V[it&1] <- V_{it-2}
        // (V_t is dead after pass A; U_{it-1}'s slot was last read in iteration it+1)
        if (t < n) {
            U[(it - 1) & 1][t] = nu;
            V[it & 1][t] = nv;
            if constexpr (WEIGHTED) { Ua[(it - 1) & 1][t] = nu - lab[0][t]; Va[it & 1][t] = nv - lab[1][t]; }
            nu = hist_u(it - 2, t);
            nv = hist_v(it - 3, t);
        }
        // (B) through u_t: column pass with P_t
        {
            const float vj = WEIGHTED ? Vp[lsafe] : Vp[lsafe] - lw2;
            float ou[EPT], og[EPT];
            load_other<EPT>(ou, WEIGHTED ? Ua[it & 1] : Uc, q);
            load_other<EPT>(og, gu, q);
            float r = 0.f;
#pragma unroll
            for (int m = 0; m < EPT; ++m) {
                const float w = __builtin_amdgcn_exp2f((ou[m] - ccol[m]) + vj) * og[m];
                dcol[m] += w;
                r += w;
            }
            r = seg_sum<LPR>(r);
            if (active && q == 0) {
                gv[line] = -r;
                if constexpr (DW) { if (it > 1) sab[1][line] += (double)(-r); }   // it == 1: the adjoint of v_0 = 0, not added
            }
        }
        lds_barrier();
    }

    if constexpr (DW) {
        const float* pa = weights_of(a.wa, a.wb, a.w_div, p, n, true);
        const float* pb = weights_of(a.wa, a.wb, a.w_div, p, n, false);
        if (t < 64) {     // (the loop's closing barrier, or the one before it, made every entry of sab visible)
            double ea = 0.0, eb = 0.0, ta = 0.0, tb = 0.0;
            for (int i = t; i < n; i += 64) { ea += sab[0][i]; eb += sab[1][i]; ta += (double)pa[i]; tb += (double)pb[i]; }
            ea = wave_sum_d(ea); eb = wave_sum_d(eb); ta = wave_sum_d(ta); tb = wave_sum_d(tb);
            if (t == 0) { mode[0] = ea / ta; mode[1] = eb / tb; }
        }
        __syncthreads();
        if (active && q == 0) {
            // da, db are read from the kernel arguments HERE, not with the others at the top: two pointers fewer in SGPRs
            // through the loop (the EPT = 16 forms are short of them too)
            const SinkBwdArgs* ka = (const SinkBwdArgs*)__builtin_amdgcn_kernarg_segment_ptr();
            const double wa = (double)pa[line], wb = (double)pb[line];
            ka->da[(int64_t)p * n + line] = (float)((double)a.eps * (sab[0][line] - mode[0] * wa) / wa);
            ka->db[(int64_t)p * n + line] = (float)((double)a.eps * (((double)gvf[line] + sab[1][line]) - mode[1] * wb) / wb);
        }
    }
    // dC = row-layout part + (column-layout part)^T
    float* dC = a.dC + (int64_t)p * n * n;
    if (active) {
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const int idx = q * EPT + m;
            if (idx < n) dC[(int64_t)line * n + idx] = drow[m];
        }
    }
    __threadfence_block();
    __syncthreads();
    if (active) {
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const int idx = q * EPT + m;
            if constexpr (EPT < 16) { if (idx < n) dC[(int64_t)idx * n + line] = canonical_nan(dC[(int64_t)idx * n + line] + dcol[m]); }
            else { if (idx < n) dC[(int64_t)idx * n + line] += dcol[m]; }
        }
    }
}

template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_bwd_reg(SinkBwdArgs a) { sinkhorn_bwd_body<EPT, LPR, false>(a); }
template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_bwd_reg_w(SinkBwdArgs a) { sinkhorn_bwd_body<EPT, LPR, true>(a); }
// the weighted sweep that also writes da, db (include/kccot_weight_grad.h)
template <int EPT, int LPR>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_bwd_reg_dw(SinkBwdArgs a) { sinkhorn_bwd_body<EPT, LPR, true, true>(a); }

// ------------------------------------------------------------------------------------------
// Fused solve + reverse sweep of the mixed divergence (compute_sinkhorn_loss when a gradient is wanted):
// ONE persistent launch per loss, one workgroup per problem, the whole dual history in LDS.
//
//   * the history row written by a half-step IS the exchange array the next half-step reads (row k of `hu` holds
//     U_k, row 0 = zeros): one ds_write per line and half-step instead of an exchange write, a global history store
//     and (shortcut build) a ring store; rows k-3 .. k are also the ring the exact periodic-state shortcut needs;
//   * the reverse sweep starts the moment the final cost is known and reads U_t / V_t / V_{t-1} straight from LDS:
//     no second launch, no reload of C (it is still in registers in both orientations), no 2*L*n-float history
//     round trip through global memory, no prefetch / refill step inside the sweep;
//   * d loss / d C is produced for dLoss = 1 with the per-problem weights of the launch: {2,-1,-1} of gan_utils.py:225
//     on three problems (compute_sinkhorn_loss), {+1,+1,-1,-1} on four (compute_mixed_sinkhorn_loss); the cost backward
//     multiplies by the upstream scalar when it builds its coefficients (the gradient is linear in it).
// Arithmetic is that of sinkhorn_fwd_body / sinkhorn_bwd_body, instruction for instruction (half_step and the shared stages
// above): costs, iteration counts and duals are bit-identical to the two-kernel path, dC to the two-kernel path at the same
// lanes-per-line.
// Eligibility (host): n <= 128 and 2 (L+1) NS floats of history within the CU's LDS; otherwise the two kernels run.
// ------------------------------------------------------------------------------------------
struct SinkFusedArgs {
    const float* C;       // [nprob,n,n], nprob = gridDim.x (3 or 4)
    int n, L, Lmin;
    float eps, inv_eps, thresh;
    float* cost_out;      // [nprob]
    int32_t* nits_out;    // [2 nprob]
    float* loss_out;      // [1] = sum_p w[p] cost[p], added left to right
    int* ticket;          // zero on entry, left zero
    float* dC;            // [nprob,n,n]
    float w[SK_FUSED_MAXPROB];   // loss weights (w[p] = +-1 or 2: every product below is exact)
    unsigned long long* diag;    // diagnostic build only (kccot_diag_fused_stamps); null otherwise
};

template <int EPT, int LPR, bool SHORTCUT, int NPROB>
__global__ __launch_bounds__(LPR * SK_MAXN < SK_MAXT ? LPR * SK_MAXN : SK_MAXT) void sinkhorn_fused_reg(SinkFusedArgs a) {
    static_assert(NPROB == 3 || NPROB == 4, "three (compute_sinkhorn_loss) or four (mixed, two minibatches) problems");
    constexpr int NS = EPT * LPR;                              // history row stride (>= n, a multiple of 4)
    extern __shared__ __attribute__((aligned(16))) float hist[];
    __shared__ __attribute__((aligned(16))) float gu[SK_MAXN + 16 * 16];
    __shared__ __attribute__((aligned(16))) float gv[SK_MAXN + 16 * 16];
    __shared__ __attribute__((aligned(16))) float red[16];
    __shared__ int mis[4];
    const int p = blockIdx.x, n = a.n, L = a.L;
    const int t = threadIdx.x, line = t / LPR, q = t % LPR;
    const bool active = line < n;
    const float* C = a.C + (int64_t)p * n * n;
    const float k2 = a.inv_eps * LOG2E;
    float* hu = hist;                                          // row k: U_k (k = 0 .. L), row 0 = 0
    float* hv = hist + (size_t)(L + 1) * NS;

    KCCOT_STAMP_IF(true, 16);                                  // 16 .. 11: the prologue
    const int nw = blockDim.x >> 6;                            // read with the kernel's other arguments, not in the tail
    // d(sum_p w[p] cost[p]) / d cost[p] at dLoss = 1.  An indexed scalar load: taken here, with the prologue's loads, so that
    // the sweep's first adjoints do not wait for it between the loops.
    const float g = a.w[p];
    float crow[EPT], ccol[EPT], craw[EPT];                     // craw: the row orientation's elements, for the final cost
    load_costs_raw<EPT, true>(C, n, line, q, k2, crow, craw);
    load_costs_raw<EPT, false>(C, n, line, q, k2, ccol);
    // row 0 and the pad columns [n, NS) of every row are zero (a pad dual pairs with c2 = +inf -> exp2(-inf) = 0)
    for (int i = t; i < NS; i += blockDim.x) { hu[i] = 0.f; hv[i] = 0.f; }
    if (NS > n) {
        const int padw = NS - n;
        for (int e = t; e < L * padw; e += blockDim.x) {
            const int k = 1 + e / padw, i = n + e % padw;
            hu[k * NS + i] = 0.f; hv[k * NS + i] = 0.f;
        }
    }
    for (int i = t; i < SK_MAXN + 16 * 16; i += blockDim.x) { gu[i] = 0.f; gv[i] = 0.f; }
    if (t < 4) mis[t] = 0;
    __syncthreads();

    const float lw2 = __builtin_amdgcn_logf(1.0f / (float)n);
    const float err_scale = a.eps * LN2;
    bool detect = SHORTCUT;
    int computed = 0;
    int mprev = ~0;
    float pu2 = 0.f, pu3 = 0.f, pu4 = 0.f, pv2 = 0.f, pv3 = 0.f, pv4 = 0.f;
    int nits = 0;
    float ui = 0.f, vj = 0.f;
    // ---------------------------------------------------------------- forward (the loop of sinkhorn_fwd_body on LDS history)
    KCCOT_STAMP_IF(true, 11);                                  // 11 .. 12: the whole forward loop
    for (int it = 0; it < L; ++it) {
        KCCOT_STAMP(9);
        const float un = half_step<EPT, LPR, true>(crow, ui, hv + it * NS, q, lw2);
        float du = 0.f;
        if (!(KCCOT_FWD_TRIM & 32) || (it + 1 >= a.Lmin && it + 1 < L)) du = (active && q == 0) ? fabsf(un - ui) : 0.f;
        int bits = 0;
        if (SHORTCUT && detect) {
            shortcut_mismatch(bits, un, ui, pu2, pu3, pu4);
            pu4 = pu3; pu3 = pu2; pu2 = ui;
        }
        ui = un;
        if (active && q == 0) hu[(it + 1) * NS + line] = un;
        lds_barrier();
        const float vn = half_step<EPT, LPR, false>(ccol, vj, hu + (it + 1) * NS, q, lw2);
        if (SHORTCUT && detect) {
            shortcut_mismatch(bits, vn, vj, pv2, pv3, pv4);
            pv4 = pv3; pv3 = pv2; pv2 = vj;
            shortcut_vote(bits, active, t, mis, it);
        }
        vj = vn;
        if (active && q == 0) hv[(it + 1) * NS + line] = vn;
        lds_barrier();
        KCCOT_STAMP(10);
        nits = it + 1;
        ++computed;
        if (nits >= a.Lmin && it + 1 < L) {                   // gan_utils.py:157-160
            const float err = block_sum(du, red) * err_scale;
            if (a.thresh > err) break;
        }
        if (SHORTCUT && detect) {
            const int per = shortcut_period(mis, it, t, mprev);
            if (per) {
                detect = false;
                const int K1 = shortcut_resume(L, a.Lmin, KCCOT_STOP_COUNT);
                if (K1 > nits) {
                    fill_history_rows(hu, hv, NS, n, t, nits, K1, per);
                    __syncthreads();
                    ui = hu[K1 * NS + (active ? line : 0)];
                    vj = hv[K1 * NS + (active ? line : 0)];
                    nits = K1;
                    it = K1 - 1;
                }
            }
        }
    }

    KCCOT_STAMP_IF(true, 12);
    const float* Vn = hv + nits * NS;
    const float* Un = hu + nits * NS;
    // The final cost is formed and handed off BEHIND the sweep, which needs neither (g = a.w[p] is a constant, nits is in a
    // register): here each wave only sums its lanes' parts, from registers and LDS.  Between the two loops there is no global
    // access, no wait for one, and one barrier (the one in front of the sweep, which the adjoints below need).
    // (<16,8>, n > 64 under option "sinkhorn_fused_max_n" = 128, runs at the 128-VGPR cap of 1024 threads and spilled before;
    // its scratch grows from 144-148 to 188-200 bytes per lane.  A form that re-read C here instead spilled as much.)
    const float psum = wave_sum(cost_partial<EPT>(crow, craw, ui, Vn, n, q, active));
    KCCOT_STAMP_IF(true, 17);

    // ---------------------------------------------------------------- reverse sweep (sinkhorn_bwd_body on LDS history)
    const int lsafe = active ? line : 0;
    float drow[EPT], dcol[EPT];
    {
        const float uf = Un[lsafe], vf = Vn[lsafe];
        float ov[EPT], ou[EPT];
        load_other<EPT>(ov, Vn, q);
        load_other<EPT>(ou, Un, q);
        float su = 0.f, sv = 0.f;
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const bool ok = active && (q * EPT + m) < n;
            final_cost_adjoint<true>(crow[m], uf, ov[m], ok, g, drow[m], su);
            final_cost_adjoint<false>(ccol[m], vf, ou[m], ok, g, dcol[m], sv);
        }
        su = seg_sum<LPR>(su);
        sv = seg_sum<LPR>(sv);
        if (active && q == 0) { gu[line] = g * su * LN2; gv[line] = g * sv * LN2; }
    }
    KCCOT_STAMP_IF(true, 20);
    lds_barrier();
    // The plans Q_t (pass A) and P_t (pass B) depend on the HISTORY only, not on the running gradients: the dependent
    // chain of a half-step is gv -> 8 multiply-adds -> DPP sum -> gu.  Their exp2 are therefore evaluated one pass
    // AHEAD, in the shadow of the LDS round trip that follows every barrier (ds_read of the gradients): the same
    // instructions, issued while the wave would otherwise wait.
    float qa[EPT], pb[EPT];
    auto plan_a = [&](int it) {      // Q_it[line][q*EPT+m] = exp2((U_it,line - lw2 - c) + V_it,col)
        const float uu = hu[it * NS + lsafe] - lw2;
        float ov[EPT];
        load_other<EPT>(ov, hv + it * NS, q);
#pragma unroll
        for (int m = 0; m < EPT; ++m) qa[m] = __builtin_amdgcn_exp2f((uu - crow[m]) + ov[m]);
    };
    auto plan_b = [&](int it) {      // P_it[q*EPT+m][line] = exp2((U_it,row - c) + V_{it-1,line} - lw2)
        const float vv = hv[(it - 1) * NS + lsafe] - lw2;
        float ou[EPT];
        load_other<EPT>(ou, hu + it * NS, q);
#pragma unroll
        for (int m = 0; m < EPT; ++m) pb[m] = __builtin_amdgcn_exp2f((ou[m] - ccol[m]) + vv);
    };
    KCCOT_STAMP_IF(true, 13);                                  // 13 .. 14: the whole sweep loop
    if (nits >= 1) plan_a(nits);
    for (int it = nits; it >= 1; --it) {
        {   // (A) through v_t: row pass with Q_t
            KCCOT_STAMP(0);
            float og[EPT];
            load_other<EPT>(og, gv, q);
            plan_b(it);
            __builtin_amdgcn_sched_barrier(0);          // keep the exp2 of the next pass in the shadow of the gv read
            KCCOT_STAMP(1);
            float sa = 0.f;
#pragma unroll
            for (int m = 0; m < EPT; ++m) {
                const float w = qa[m] * og[m];
                drow[m] += w;
                sa += w;
            }
            sa = seg_sum<LPR>(sa);
            KCCOT_STAMP(2);
            if (active && q == 0) gu[line] = (it == nits ? gu[line] : 0.f) - sa;
            KCCOT_STAMP(3);
        }
        lds_barrier();
        {   // (B) through u_t: column pass with P_t
            KCCOT_STAMP(4);
            float og[EPT];
            load_other<EPT>(og, gu, q);
            if (it > 1) plan_a(it - 1);
            __builtin_amdgcn_sched_barrier(0);
            KCCOT_STAMP(5);
            float r = 0.f;
#pragma unroll
            for (int m = 0; m < EPT; ++m) {
                const float w = pb[m] * og[m];
                dcol[m] += w;
                r += w;
            }
            r = seg_sum<LPR>(r);
            KCCOT_STAMP(6);
            if (active && q == 0) gv[line] = -r;
            KCCOT_STAMP(7);
        }
        lds_barrier();
        KCCOT_STAMP(8);
    }
    KCCOT_STAMP_IF(true, 14);
    float* dC = a.dC + (int64_t)p * n * n;
    // dC through the LDS tile (park_dc_cols), and the waves' cost sums with it: one barrier, every row stored once, no global
    // load.  Thread 0 hands the cost off last, behind its own row stores: its drain waits for stores the kernel's end waits
    // for anyway, and no other wave waits for thread 0 any more.
    park_dc_cols<EPT>(hist, dcol, n, line, q, active);
    if ((t & 63) == 0) red[t >> 6] = psum;
    lds_barrier();
    KCCOT_STAMP_IF(true, 21);
    take_dc_cols<EPT>(hist, drow, n, line, q, active);
    store_dc_rows<EPT>(dC, drow, n, line, q, active);
    if (t == 0) publish_cost<NPROB>(a.cost_out, a.nits_out, a.loss_out, a.ticket, p, canonical_nan(cost_of_waves(red, nw)), nits, computed, a.w, true);
    KCCOT_STAMP_IF(true, 19);
    KCCOT_STAMP_DRAINED(22);
}

// ------------------------------------------------------------------------------------------
// sinkhorn_fused_roles: sinkhorn_fused_reg with the two orientations on SEPARATE waves (option "sinkhorn_fused_roles").
//
// In sinkhorn_fused_reg every wave holds the costs in both orientations and runs both passes of every iteration, so in
// the reverse sweep the plan of the NEXT pass (8 packed adds + 8 exp2 per lane, independent of the running gradients) is
// issued by the very wave whose multiply-add chain the workgroup is waiting for.  Here the workgroup is 2 TR threads,
// TR = ceil64(n LPR): threads [0, TR) are the ROW role (row orientation: ui, pass A, plan_a), threads [TR, 2 TR) the
// COLUMN role (column orientation: vj, pass B, plan_b).  The role is wave-uniform.  While one role is on the chain the
// other evaluates its next plan, then both meet at the barrier that was there anyway: same two barriers per iteration,
// same gu / gv and history exchange through LDS, nothing else shared.
//
// Bit-identical to sinkhorn_fused_reg: lane (line, q) of a role executes, on the same operands and in the same order, the
// instructions that lane (line, q) of the one-role kernel executes for that orientation; the plans never leave the
// registers of the wave that consumes them; the block sums (stop rule, cost) add the waves in order and the column waves
// contribute trailing + 0.0f terms to a sum that starts at + 0.0f.  Every wave executes the same number of barriers on
// every path (both roles run the same loop with the same wave-uniform trip counts; only the work between barriers differs).
// Host: taken when 2 TR <= 1024 (kccot_sinkhorn_fused_roles_eligible); otherwise sinkhorn_fused_reg runs.
// ------------------------------------------------------------------------------------------
// Wave priority in the reverse sweep.  The two roles share every SIMD (two waves of each in the 1024-thread
// instances) and the SIMD's vector port goes to the higher priority, then to the older wave: at equal priority the row
// role's waves (the older ones) win it in both passes, and the column role's chain, which the whole workgroup waits for in
// pass B, gets the slots the row role's plan leaves.  So the role that is on the chain runs its pass raised and drops to 0 in
// front of the barrier that ends it; the role evaluating its plan runs at 0.  s_setprio is a scalar instruction that ignores
// EXEC: the role is a template parameter, so each instantiation carries its own unconditional pair.
// KCCOT_SWEEP_PRIO selects the form for experiment builds (profiles/sinkhorn_sweep_priority_ab.json): 0 none, 1 the chain
// pass raised in both roles (the product: -4.5 us), 2 in the column role only (-3.2 us), 3 the column role raised for the
// whole sweep (+1.9 us: the penalty only moves to pass A).  Levels 1, 2 and 3 measure the same.
#ifndef KCCOT_SWEEP_PRIO
#define KCCOT_SWEEP_PRIO 1
#endif
#ifndef KCCOT_SWEEP_PRIO_LEVEL
#define KCCOT_SWEEP_PRIO_LEVEL 1
#endif
template <bool ON>
__device__ __forceinline__ void sweep_prio(bool raised) {
    if constexpr (ON) {
        if (raised) __builtin_amdgcn_s_setprio(KCCOT_SWEEP_PRIO_LEVEL); else __builtin_amdgcn_s_setprio(0);
    }
}

template <int EPT, int LPR, bool SHORTCUT, int NPROB, bool COL>
__device__ __forceinline__ void fused_roles_body(const SinkFusedArgs& a, float* hist, float* gu, float* gv, float* red,
                                                 int* mis, const int TR) {
    constexpr int NS = EPT * LPR;
    const int p = blockIdx.x, n = a.n, L = a.L;
    const int t = threadIdx.x, tr = t - (COL ? TR : 0), line = tr / LPR, q = tr % LPR;
    const bool active = line < n;
    const float* C = a.C + (int64_t)p * n * n;
    const float k2 = a.inv_eps * LOG2E;
    float* hu = hist;
    float* hv = hist + (size_t)(L + 1) * NS;
    // this role's duals and the other role's: the row role owns U (reads V), the column role owns V (reads U)
    float* hs = COL ? hv : hu;
    const float* ho = COL ? hu : hv;

    KCCOT_STAMP_IF(true, 16);
    float c2[EPT];                                             // C * k2 in this role's orientation (load_costs)
    float craw[EPT];                                           // the elements themselves: the row role's, for the final cost
    const float g = a.w[p];                                    // loaded here, not between the loops (see sinkhorn_fused_reg)
    load_costs_raw<EPT, !COL>(C, n, line, q, k2, c2, craw);
    // row 0, the pad columns, gu / gv and mis zeroed, by every thread of both roles (the prologue of sinkhorn_fused_reg)
    for (int i = t; i < NS; i += blockDim.x) { hu[i] = 0.f; hv[i] = 0.f; }
    if (NS > n) {
        const int padw = NS - n;
        for (int e = t; e < L * padw; e += blockDim.x) {
            const int k = 1 + e / padw, i = n + e % padw;
            hu[k * NS + i] = 0.f; hv[k * NS + i] = 0.f;
        }
    }
    for (int i = t; i < SK_MAXN + 16 * 16; i += blockDim.x) { gu[i] = 0.f; gv[i] = 0.f; }
    if (t < 4) mis[t] = 0;
    __syncthreads();

    const float lw2 = __builtin_amdgcn_logf(1.0f / (float)n);
    const float err_scale = a.eps * LN2;
    bool detect = SHORTCUT;
    int computed = 0;
    int mprev = ~0;
    float p2 = 0.f, p3 = 0.f, p4 = 0.f;
    int nits = 0;
    float self = 0.f;                                          // ui (row role) / vj (column role)
    // One half-step of this role: the dual, its history row (the next half-step's exchange array) and the shortcut's
    // mismatch bits, OR-ed into mis[] per wave (both roles vote, each with the bits of its own dual).
    // In the forward only one role works per half-step and all 16 waves wait for its eight, two to a SIMD and one vector port:
    // every instruction between the barrier that opens a role's half-step and the barrier that ends it is paid by the whole
    // workgroup (tools/forward_issue_budget.py counts them).  So what the half-step does not need is done in the OTHER
    // role's half-step (off_chain), pinned between that half-step's two barriers:
    //   - the addresses of the row read and the row written are running LDS addresses (rb, wb), moved on by one row there,
    //     not it * NS formed behind the barrier in front of the read and in front of the write;
    //   - |du| (the stop rule's term, row role) is formed there too, and only in an iteration whose stop rule reads it.
    // The instances with the shortcut keep the parent's forms: there these cost two to four registers, and a solve that
    // jumps leaves this loop after a handful of iterations.
    constexpr bool RUNNING = (KCCOT_FWD_TRIM & 4) && !SHORTCUT;
    constexpr bool DU_OFF_CHAIN = (KCCOT_FWD_TRIM & 2) && !SHORTCUT;
    constexpr bool PAIRS = (KCCOT_FWD_TRIM & 16) && !SHORTCUT;
    constexpr bool ONE_MAX = (KCCOT_FWD_TRIM & 1) != 0;      // every role instance; the other callers of half_step keep seg_max
    unsigned rb = lds_address(ho + (COL ? NS : 0) + q * EPT);  // this lane's entries of the row the next half-step reads
    unsigned wb = lds_address(hs + NS + line);                 // the line's word of the row it writes
    float prev = 0.f;                                          // the dual before the last half-step
    auto own_half_step = [&](int it, float& du) {
        (void)du;
        const float* other = RUNNING ? lds_pointer(rb) : ho + (COL ? it + 1 : it) * NS + q * EPT;
        const float sn = half_step<EPT, LPR, !COL, PAIRS, ONE_MAX>(c2, self, other, 0, lw2, [&](int k) { (void)k; KCCOT_STAMP(24 + k); });
        if constexpr (!DU_OFF_CHAIN) du = (active && q == 0) ? fabsf(sn - self) : 0.f;
        if (active && q == 0) {
            if constexpr (RUNNING) *lds_pointer(wb) = sn;
            else hs[(it + 1) * NS + line] = sn;
        }
        KCCOT_STAMP(26);
        if (SHORTCUT && detect) {
            int bits = 0;
            shortcut_mismatch(bits, sn, self, p2, p3, p4);
            p4 = p3; p3 = p2; p2 = self;
            shortcut_vote(bits, active, t, mis, it);
        }
        if constexpr (DU_OFF_CHAIN) prev = self;
        self = sn;
    };
    // this role's work of the half-step in which the other role is on the chain; the empty asm statements hold it between
    // the two barriers around them (a barrier orders memory operations, not register arithmetic: see keep_in_regs)
    auto off_chain = [&](int it, float& du) {
        if constexpr (RUNNING) asm volatile("" : "+v"(self), "+v"(rb), "+v"(wb));
        if constexpr (DU_OFF_CHAIN && !COL) {
            if (it + 1 >= a.Lmin && it + 1 < L) du = (active && q == 0) ? fabsf(self - prev) : 0.f;
        }
        if constexpr (RUNNING) {
            rb += NS * 4; wb += NS * 4;
            asm volatile("" : "+v"(rb), "+v"(wb));
        }
    };
    // ---------------------------------------------------------------- forward
    KCCOT_STAMP_IF(true, 11);
    for (int it = 0; it < L; ++it) {
        KCCOT_STAMP(9);
        float du = 0.f;
        if constexpr (!COL) own_half_step(it, du);
        lds_barrier();
        KCCOT_STAMP(27);
        if constexpr (COL) { float dv; own_half_step(it, dv); }
        else off_chain(it, du);
        lds_barrier();
        KCCOT_STAMP(10);
        if constexpr (COL) { float dv; off_chain(it, dv); }
        nits = it + 1;
        ++computed;
        if (nits >= a.Lmin && it + 1 < L) {                   // gan_utils.py:157-160 (sum over the row role's du)
            const float err = block_sum(du, red) * err_scale;
            if (a.thresh > err) break;
        }
        if (SHORTCUT && detect) {
            const int per = shortcut_period(mis, it, t, mprev);
            if (per) {
                detect = false;
                const int K1 = shortcut_resume(L, a.Lmin, KCCOT_STOP_COUNT);
                if (K1 > nits) {                              // (no running addresses to move: RUNNING implies !SHORTCUT)
                    fill_history_rows(hu, hv, NS, n, t, nits, K1, per);
                    __syncthreads();
                    self = hs[K1 * NS + (active ? line : 0)];
                    nits = K1;
                    it = K1 - 1;
                }
            }
        }
    }

    KCCOT_STAMP_IF(true, 12);
    // the final cost: the row role's lanes, zeros from the others
    const float* Vn = hv + nits * NS;
    const float* Un = hu + nits * NS;
    // formed and handed off behind the sweep (see sinkhorn_fused_reg): no global access, no wait for one and one barrier
    // between the two loops
    float psum = 0.f;
    if constexpr (!COL) psum = wave_sum(cost_partial<EPT>(c2, craw, self, Vn, n, q, active));
    KCCOT_STAMP_IF(true, 17);

    // ---------------------------------------------------------------- reverse sweep
    const int lsafe = active ? line : 0;
    float d[EPT];                                              // drow (row role) / dcol (column role)
    {
        const float sf = (COL ? Vn : Un)[lsafe];
        float oo[EPT];
        load_other<EPT>(oo, COL ? Un : Vn, q);
        float ss = 0.f;
#pragma unroll
        for (int m = 0; m < EPT; ++m) final_cost_adjoint<!COL>(c2[m], sf, oo[m], active && (q * EPT + m) < n, g, d[m], ss);
        ss = seg_sum<LPR>(ss);
        if (active && q == 0) (COL ? gv : gu)[line] = g * ss * LN2;
    }
    KCCOT_STAMP_IF(true, 20);
    lds_barrier();
    float pl[EPT];                                             // Q_t (row role, plan_a) / P_t (column role, plan_b)
    auto plan = [&](int it) {
        // row:    Q_it[line][q*EPT+m] = exp2((U_it,line - lw2 - c) + V_it,col)
        // column: P_it[q*EPT+m][line] = exp2((U_it,row - c) + V_{it-1,line} - lw2)
        const float sv = hs[(COL ? it - 1 : it) * NS + lsafe] - lw2;
        float oo[EPT];
        load_other<EPT>(oo, ho + it * NS, q);
#pragma unroll
        for (int m = 0; m < EPT; ++m) pl[m] = __builtin_amdgcn_exp2f(COL ? ((oo[m] - c2[m]) + sv) : ((sv - c2[m]) + oo[m]));
    };
    // this role's pass: the gradients the other role wrote -> multiply-adds -> DPP sum -> this role's gradients
    auto chain = [&](int it) {
        float og[EPT];
        load_other<EPT>(og, COL ? gu : gv, q);
        KCCOT_STAMP(COL ? 5 : 1);
        float s = 0.f;
#pragma unroll
        for (int m = 0; m < EPT; ++m) {
            const float w = pl[m] * og[m];
            d[m] += w;
            s += w;
        }
        s = seg_sum<LPR>(s);
        KCCOT_STAMP(COL ? 6 : 2);
        if (active && q == 0) {
            if constexpr (COL) gv[line] = -s;
            else gu[line] = (it == nits ? gu[line] : 0.f) - s;
        }
        KCCOT_STAMP(COL ? 7 : 3);
    };
    KCCOT_STAMP_IF(true, 13);
    // Every plan is pinned (keep_in_regs) in front of the barrier that ends the pass it is evaluated in: the chain pass behind
    // that barrier then holds the gradient read and the chain, and no plan arithmetic (tests/test_fused_roles_schedule.py
    // checks the emitted code of every instance).  The stamps of the diagnostic twin are taken behind the pinned registers, so
    // that they time the plan and not only its loads.
    if constexpr (!COL) { if (nits >= 1) { plan(nits); keep_in_regs(pl); } }
    if constexpr (COL) sweep_prio<KCCOT_SWEEP_PRIO == 3>(true);
    for (int it = nits; it >= 1; --it) {
        KCCOT_STAMP(0);
        if constexpr (COL) { plan(it); keep_in_regs(pl); KCCOT_STAMP(1); }                             // (A) through v_t
        else { sweep_prio<KCCOT_SWEEP_PRIO == 1>(true); chain(it); sweep_prio<KCCOT_SWEEP_PRIO == 1>(false); }
        lds_barrier();
        KCCOT_STAMP(4);
        if constexpr (COL) { sweep_prio<KCCOT_SWEEP_PRIO == 1 || KCCOT_SWEEP_PRIO == 2>(true); chain(it); sweep_prio<KCCOT_SWEEP_PRIO == 1 || KCCOT_SWEEP_PRIO == 2>(false); }
        else { if (it > 1) { plan(it - 1); keep_in_regs(pl); } KCCOT_STAMP(5); }                           // (B) through u_t
        lds_barrier();
        KCCOT_STAMP(8);
    }
    if constexpr (COL) sweep_prio<KCCOT_SWEEP_PRIO == 3>(false);
    KCCOT_STAMP_IF(true, 14);
    float* dC = a.dC + (int64_t)p * n * n;
    // dC through the LDS tile, the waves' cost sums with it (the column waves' + 0.0f keep block_sum's sum): one barrier.
    // Behind it the row role adds the transposed entries and stores every row once; the column role has nothing left to do,
    // so its first thread forms the cost and hands it off while the rows are stored.  No wave waits for that thread.
    if constexpr (COL) park_dc_cols<EPT>(hist, d, n, line, q, active);
    if ((t & 63) == 0) red[t >> 6] = psum;
    lds_barrier();
    KCCOT_STAMP_IF(true, 21);
    if constexpr (!COL) {
        take_dc_cols<EPT>(hist, d, n, line, q, active);
        store_dc_rows<EPT>(dC, d, n, line, q, active);
    } else {
        if (tr == 0) publish_cost<NPROB>(a.cost_out, a.nits_out, a.loss_out, a.ticket, p, canonical_nan(cost_of_waves(red, TR >> 5)), nits, computed, a.w, true);
        KCCOT_STAMP_IF(true, 19);
    }
    KCCOT_STAMP_DRAINED(22);
}

template <int EPT, int LPR, bool SHORTCUT, int NPROB>
__global__ __launch_bounds__(SK_MAXT) void sinkhorn_fused_roles(SinkFusedArgs a) {
    static_assert(NPROB == 3 || NPROB == 4, "three (compute_sinkhorn_loss) or four (mixed, two minibatches) problems");
    extern __shared__ __attribute__((aligned(16))) float hist[];
    __shared__ __attribute__((aligned(16))) float gu[SK_MAXN + 16 * 16];
    __shared__ __attribute__((aligned(16))) float gv[SK_MAXN + 16 * 16];
    __shared__ __attribute__((aligned(16))) float red[16];
    __shared__ int mis[4];
    const int TR = blockDim.x >> 1;                            // threads per role, a multiple of 64: the role is wave-uniform
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x >= TR)) fused_roles_body<EPT, LPR, SHORTCUT, NPROB, true>(a, hist, gu, gv, red, mis, TR);
    else fused_roles_body<EPT, LPR, SHORTCUT, NPROB, false>(a, hist, gu, gv, red, mis, TR);
}

// gan_utils.py:225: loss = 2.0 * loss_xy - loss_xx - loss_yy, evaluated left to right in fp32
__global__ void mixed_divergence_fwd(const float* __restrict__ cost3, float* __restrict__ loss) {
    if (threadIdx.x == 0) loss[0] = (2.0f * cost3[0] - cost3[1]) - cost3[2];
}
__global__ void mixed_divergence_bwd(const float* __restrict__ gloss, float* __restrict__ gcost3) {
    if (threadIdx.x == 0) {
        const float g = gloss[0];
        gcost3[0] = 2.0f * g; gcost3[1] = -g; gcost3[2] = -g;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
struct SinkGeom { int lpr, ept, threads; };

static SinkGeom sink_geom(int n, bool forward) {
    SinkGeom g;
    // n*lpr <= 1024.  Every wave of the workgroup runs the same instruction stream between two
    // barriers, four waves take turns on each SIMD at 1024 threads, and the per-wave overhead (DPP
    // reduction steps, log, stores) does not shrink with the number of entries per lane.  Measured
    // at n = 64 over 100 iterations (tools/bench_sinkhorn.py, tools/ab_sk.sh): forward 8 lanes per
    // line 72 us, 16: 82 us, 4: slower still; the reverse sweep is within 2 us between 8 and 16
    // (72 us) and keeps 16.
    g.lpr = (n <= 32) ? 16 : (n <= 64 ? (forward ? 8 : 16) : 8);
    if (n > 32 && n <= 64) {
        // option "sinkhorn_lanes_per_line" = 4, 8 or 16 (0 = the rule above): the fused kernel runs 8, so equality tests of
        // its gradients against the two-kernel path put both on 8
        const int v = opt(OPT_SK_LPR);
        if (v == 4 || v == 8 || v == 16) g.lpr = v;
    }
    const int need = (n + g.lpr - 1) / g.lpr;
    g.ept = need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : need <= 8 ? 8 : 16;
    g.threads = (n * g.lpr + 63) / 64 * 64;
    return g;
}

}  // namespace kccot

namespace kccot {
// sinkhorn_gen.hip: streaming kernels for 128 < n <= 1024
size_t sinkhorn_gen_workspace_bytes(int nprob, int n);
int launch_sinkhorn_fwd_gen(const float* C, int nprob, int n, float eps, int L, int Lmin, float thresh, int stop_mode,
                            float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out, float* pi_out, void* ws,
                            size_t ws_bytes, hipStream_t st, const float* wa, const float* wb, int w_div);
int launch_sinkhorn_bwd_gen(const float* C, const float* u_hist, const float* v_hist, const int32_t* nits, int nprob, int n,
                            float eps, int L, const float* gcost, float* dC, void* ws, size_t ws_bytes, hipStream_t st,
                            const float* wa, const float* wb, int w_div, float* da, float* db);
}  // namespace kccot

using namespace kccot;

// option "sinkhorn_shortcut" = 0: always execute every iteration (bench headline, bitwise-equality tests)
static int sink_shortcut_enabled() { return opt(OPT_SK_SHORTCUT); }

extern "C" size_t kccot_sinkhorn_workspace_bytes(int nprob, int n) {
    if (nprob <= 0 || n <= SK_MAXN) return 0;   // the register-resident kernels need none
    return sinkhorn_gen_workspace_bytes(nprob, n);
}

#define KCCOT_SK_LAUNCH(KERNEL, E, P, ARGS, GEOM, NPROB, ST) \
    hipLaunchKernelGGL((KERNEL<E, P>), dim3(NPROB), dim3((GEOM).threads), 0, ST, ARGS)

#define KCCOT_SK_DISPATCH(KERNEL, ARGS, GEOM, NPROB, ST)                                       \
    if ((GEOM).lpr == 16) {                                                                    \
        switch ((GEOM).ept) {                                                                  \
            case 1: KCCOT_SK_LAUNCH(KERNEL, 1, 16, ARGS, GEOM, NPROB, ST); break;              \
            case 2: KCCOT_SK_LAUNCH(KERNEL, 2, 16, ARGS, GEOM, NPROB, ST); break;              \
            default: KCCOT_SK_LAUNCH(KERNEL, 4, 16, ARGS, GEOM, NPROB, ST); break;             \
        }                                                                                      \
    } else if ((GEOM).lpr == 4) {                                                              \
        KCCOT_SK_LAUNCH(KERNEL, 16, 4, ARGS, GEOM, NPROB, ST);                                 \
    } else {                                                                                   \
        switch ((GEOM).ept) {                                                                  \
            case 8: KCCOT_SK_LAUNCH(KERNEL, 8, 8, ARGS, GEOM, NPROB, ST); break;               \
            default: KCCOT_SK_LAUNCH(KERNEL, 16, 8, ARGS, GEOM, NPROB, ST); break;             \
        }                                                                                      \
    }

// div_loss / div_ticket: the loss and the arrival counter of the divergence forward's in-kernel combine
// (kccot_sinkhorn_divergence_fwd_f32); null for the plain solves.  wa / wb / w_div: weighted marginals (SinkArgs), both
// null for mu = nu = 1/n.  Weighted solves run the register kernels (n <= 128) or the streaming single-workgroup solver,
// never the multi-CU one.
static int sinkhorn_fwd(const float* C, int nprob, int n, float eps, int L, int Lmin, float thresh, int stop_mode,
                        float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out, float* pi_out, void* ws,
                        size_t ws_bytes, kccot_stream_t stream, float* div_loss, int* div_ticket,
                        const float* wa = nullptr, const float* wb = nullptr, int w_div = 0) {
    if (!C || !cost_out || !nits_out) return fail(KCCOT_EINVAL, "sinkhorn_fwd: null pointer");
    if ((wa == nullptr) != (wb == nullptr)) return fail(KCCOT_EINVAL, "sinkhorn_fwd: give both weight vectors or neither");
    if (w_div == 1 && nprob != 3) return fail(KCCOT_EINVAL, "sinkhorn_fwd: the divergence's weights need nprob = 3");
    if (w_div == 2 && nprob % 3) return fail(KCCOT_EINVAL, "sinkhorn_fwd: the conditional mode needs nprob = 3 Q");
    if (nprob <= 0 || n <= 0 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "sinkhorn_fwd: bad arguments nprob=%d n=%d L=%d eps=%g", nprob, n, L, (double)eps);
    if ((u_hist == nullptr) != (v_hist == nullptr))
        return fail(KCCOT_EINVAL, "sinkhorn_fwd: u_hist and v_hist must be given together");
    if (stop_mode != KCCOT_STOP_COUNT && stop_mode != KCCOT_STOP_INDEX)
        return fail(KCCOT_EINVAL, "sinkhorn_fwd: bad stop_mode %d", stop_mode);
    if (n > SK_MAXN)
        return launch_sinkhorn_fwd_gen(C, nprob, n, eps, L, Lmin, thresh, stop_mode, u_hist, v_hist, cost_out, nits_out,
                                       pi_out, ws, ws_bytes, (hipStream_t)stream, wa, wb, w_div);
    SinkGeom g = sink_geom(n, true);
    SinkArgs a{C, n, L, Lmin, stop_mode, eps, (float)(1.0 / (double)eps), thresh, u_hist, v_hist, cost_out, nits_out, pi_out,
               nullptr, div_loss, div_ticket, sink_shortcut_enabled(), wa, wb, w_div};
#ifdef KCCOT_DIAG
    a.diag = static_cast<unsigned long long*>(ws);   // diagnostic build: ws carries the stamp buffer
#endif
    hipStream_t st = (hipStream_t)stream;
    if (wa) {
        if (a.shortcut) {
            KCCOT_SK_DISPATCH(sinkhorn_fwd_reg_w, a, g, nprob, st)
        } else {
            KCCOT_SK_DISPATCH(sinkhorn_fwd_reg_full_w, a, g, nprob, st)
        }
        return launch_status("sinkhorn_fwd_reg_w");
    }
    if (a.shortcut) {
        KCCOT_SK_DISPATCH(sinkhorn_fwd_reg, a, g, nprob, st)
    } else {
        KCCOT_SK_DISPATCH(sinkhorn_fwd_reg_full, a, g, nprob, st)
    }
    return launch_status("sinkhorn_fwd_reg");
}

extern "C" int kccot_sinkhorn_fwd_f32(const float* C, int nprob, int n, float eps, int L, int Lmin,
                                      float thresh, int stop_mode, float* u_hist, float* v_hist,
                                      float* cost_out, int32_t* nits_out, float* pi_out, void* ws,
                                      size_t ws_bytes, kccot_stream_t stream) {
    return sinkhorn_fwd(C, nprob, n, eps, L, Lmin, thresh, stop_mode, u_hist, v_hist, cost_out, nits_out, pi_out, ws,
                        ws_bytes, stream, nullptr, nullptr);
}

extern "C" int kccot_sinkhorn_status(const int32_t* nits, int nprob, kccot_stream_t stream) {
    if (!nits || nprob <= 0 || nprob > 4096) return fail(KCCOT_EINVAL, "sinkhorn_status: bad arguments");
    int32_t host[4096];
    hipStream_t st = (hipStream_t)stream;
    if (hipMemcpyAsync(host, nits, sizeof(int32_t) * nprob, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(KCCOT_EINVAL, "sinkhorn_status: could not read the iteration counts");
    for (int p = 0; p < nprob; ++p)
        if (host[p] < 0)
            return fail(KCCOT_EABORTED, "sinkhorn: problem %d of %d was aborted -- a workgroup of the multi-CU solver never "
                        "arrived (device shared or partitioned?); set KCCOT_SK_NO_COOP=1 to use the one-workgroup solver", p, nprob);
    return 0;
}

// div_weights = 1: gcost is ONE float dLoss/dloss and the sweep applies the weights {2,-1,-1} of the divergence
// (kccot_sinkhorn_divergence_bwd_f32); 0: gcost holds one float per problem
static int sinkhorn_bwd(const float* C, const float* u_hist, const float* v_hist, const int32_t* nits, int nprob, int n,
                        float eps, int L, const float* gcost, float* dC_out, void* ws, size_t ws_bytes,
                        kccot_stream_t stream, int div_weights, const float* wa = nullptr, const float* wb = nullptr,
                        int w_div = 0, float* da = nullptr, float* db = nullptr) {
    if (!C || !u_hist || !v_hist || !nits || !gcost || !dC_out)
        return fail(KCCOT_EINVAL, "sinkhorn_bwd: null pointer");
    if ((da == nullptr) != (db == nullptr) || (da && !wa))
        return fail(KCCOT_EINVAL, "sinkhorn_bwd: da and db are given together, with the weights");
    if ((wa == nullptr) != (wb == nullptr)) return fail(KCCOT_EINVAL, "sinkhorn_bwd: give both weight vectors or neither");
    if (w_div == 1 && nprob != 3) return fail(KCCOT_EINVAL, "sinkhorn_bwd: the divergence's weights need nprob = 3");
    if (w_div == 2 && nprob % 3) return fail(KCCOT_EINVAL, "sinkhorn_bwd: the conditional mode needs nprob = 3 Q");
    if (nprob <= 0 || n <= 0 || L < 0 || !(eps > 0.f))
        return fail(KCCOT_EINVAL, "sinkhorn_bwd: bad arguments nprob=%d n=%d L=%d eps=%g", nprob, n, L, (double)eps);
    if (n > SK_MAXN)
        return launch_sinkhorn_bwd_gen(C, u_hist, v_hist, nits, nprob, n, eps, L, gcost, dC_out, ws, ws_bytes,
                                       (hipStream_t)stream, wa, wb, w_div, da, db);
    SinkGeom g = sink_geom(n, false);
    SinkBwdArgs a{C, u_hist, v_hist, nits, gcost, dC_out, n, L, eps, (float)(1.0 / (double)eps), div_weights, wa, wb, w_div,
                  da, db};
    hipStream_t st = (hipStream_t)stream;
    if (da) {
        KCCOT_SK_DISPATCH(sinkhorn_bwd_reg_dw, a, g, nprob, st)
        return launch_status("sinkhorn_bwd_reg_dw");
    }
    if (wa) {
        KCCOT_SK_DISPATCH(sinkhorn_bwd_reg_w, a, g, nprob, st)
        return launch_status("sinkhorn_bwd_reg_w");
    }
    KCCOT_SK_DISPATCH(sinkhorn_bwd_reg, a, g, nprob, st)
    return launch_status("sinkhorn_bwd_reg");
}

extern "C" int kccot_sinkhorn_bwd_f32(const float* C, const float* u_hist, const float* v_hist,
                                      const int32_t* nits, int nprob, int n, float eps, int L,
                                      const float* gcost, float* dC_out, void* ws, size_t ws_bytes,
                                      kccot_stream_t stream) {
    return sinkhorn_bwd(C, u_hist, v_hist, nits, nprob, n, eps, L, gcost, dC_out, ws, ws_bytes, stream, 0);
}

extern "C" int kccot_mixed_divergence_fwd_f32(const float* cost3, float* loss_out, kccot_stream_t stream) {
    if (!cost3 || !loss_out) return fail(KCCOT_EINVAL, "mixed_divergence_fwd: null pointer");
    hipLaunchKernelGGL(mixed_divergence_fwd, dim3(1), dim3(64), 0, (hipStream_t)stream, cost3, loss_out);
    return launch_status("mixed_divergence_fwd");
}

extern "C" int kccot_mixed_divergence_bwd_f32(const float* gloss, float* gcost3_out, kccot_stream_t stream) {
    if (!gloss || !gcost3_out) return fail(KCCOT_EINVAL, "mixed_divergence_bwd: null pointer");
    hipLaunchKernelGGL(mixed_divergence_bwd, dim3(1), dim3(64), 0, (hipStream_t)stream, gloss, gcost3_out);
    return launch_status("mixed_divergence_bwd");
}

// ---- fused solve + reverse sweep (sinkhorn_fused_reg) -------------------------------------------------
#ifdef KCCOT_DIAG
// diagnostic twin only (tools/diag_sinkhorn.py): the device buffer [nprob,16 waves,KCCOT_DIAG_SLOTS] that the fused kernels stamp
static unsigned long long* g_fused_stamps = nullptr;
extern "C" void kccot_diag_fused_stamps(void* buf) { g_fused_stamps = static_cast<unsigned long long*>(buf); }
#endif
static size_t fused_hist_bytes(int n, int L) {
    const SinkGeom g = sink_geom(n, true);
    return (size_t)2 * ((size_t)L + 1) * g.lpr * g.ept * sizeof(float);
}
// the dynamic LDS of a fused launch: the history, or the n x (n + 1) tile of the dC transpose that takes its place behind
// the sweep (park_dc_cols), whichever is larger -- at L = 1 the history is 1 KB and the tile 16 KB.  The tile is at most
// 128 x 129 floats = 64.5 KB, so it never adds to what the eligibility rule admits.
static size_t fused_lds_bytes(int n, int L) {
    const size_t hist = fused_hist_bytes(n, L), tile = (size_t)n * ((size_t)n + 1) * sizeof(float);
    return hist > tile ? hist : tile;
}

extern "C" int kccot_sinkhorn_fused_eligible(int n, int L) {
    if (!opt(OPT_SK_FUSED)) return 0;                     // option "sinkhorn_fused" = 0: always the two-kernel path
    // n <= 64 by default: at 64 < n <= 128 (16 entries per lane and orientation) the fused kernel spills under the
    // 128-VGPR cap of a 1024-thread workgroup and measured SLOWER than the two kernels at configs[2]
    // (1.24 vs 1.08 ms per loss); option "sinkhorn_fused_max_n" = 128 re-enables it.
    const int maxn = opt(OPT_SK_FUSED_MAX_N);
    if (n <= 0 || n > SK_MAXN || n > maxn || L < 0) return 0;
    return fused_hist_bytes(n, L) <= (size_t)144 * 1024;  // + ~4 KB of static LDS, inside the CU's 160 KB
}

// The role-split kernel (sinkhorn_fused_roles) doubles the workgroup: it is taken where option "sinkhorn_fused_roles" is set,
// the one-role kernel is eligible and both roles fit one workgroup, 2 ceil64(n lanes) <= 1024: n <= 32 at 16 lanes per
// line, n <= 64 at 8 or 4.  (<4,16> and <16,8> never fit; every instance that does is scratch-free under the 128-VGPR cap
// of 1024 threads, see profiles/sinkhorn_roles_ab.json.)
extern "C" int kccot_sinkhorn_fused_roles_eligible(int n, int L) {
    if (!opt(OPT_SK_FUSED_ROLES) || !kccot_sinkhorn_fused_eligible(n, L)) return 0;
    return 2 * sink_geom(n, true).threads <= SK_MAXT;
}

// one workgroup of `threads` per problem, the history and then the dC tile in `lds` bytes of dynamic LDS (fused_lds_bytes)
// (`what` heads the error text, `name` is the kernel's name for launch_status)
static int launch_fused_kernel(void (*kernel)(SinkFusedArgs), int threads, const char* what, const char* name, int nprob,
                               const SinkFusedArgs& a, size_t lds, hipStream_t st) {
    // on every launch: the attribute belongs to the current device's copy of the function (a per-process "done" flag
    // would be wrong on a second device and racy between threads); it is a host-side table write
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 144 * 1024) !=
        hipSuccess)
        return fail(KCCOT_EUNSUPPORTED, "%s: cannot raise the dynamic LDS limit", what);
    hipLaunchKernelGGL(kernel, dim3(nprob), dim3(threads), lds, st, a);
    return launch_status(name);
}

template <int EPT, int LPR, bool SC, int NP>
static int launch_fused_np(const SinkFusedArgs& a, size_t lds, hipStream_t st) {
    const int tr = (a.n * LPR + 63) / 64 * 64;
    if (kccot_sinkhorn_fused_roles_eligible(a.n, a.L)) {
        if constexpr ((EPT == 4 && LPR == 16) || (EPT == 16 && LPR == 8))
            return fail(KCCOT_EUNSUPPORTED, "sinkhorn_fused_roles: no <%d,%d> instance", EPT, LPR);
        else
            return launch_fused_kernel(sinkhorn_fused_roles<EPT, LPR, SC, NP>, 2 * tr, "sinkhorn_fused_roles", "sinkhorn_fused_roles", NP,
                                       a, lds, st);
    }
    return launch_fused_kernel(sinkhorn_fused_reg<EPT, LPR, SC, NP>, tr, "sinkhorn_fused", "sinkhorn_fused_reg", NP, a, lds, st);
}

template <int EPT, int LPR, bool SC>
static int launch_fused(const SinkFusedArgs& a, int nprob, size_t lds, hipStream_t st) {
    return nprob == 3 ? launch_fused_np<EPT, LPR, SC, 3>(a, lds, st) : launch_fused_np<EPT, LPR, SC, 4>(a, lds, st);
}

template <bool SC>
static int dispatch_fused(const SinkGeom& g, const SinkFusedArgs& a, int nprob, size_t lds, hipStream_t st) {
    if (g.lpr == 16) {
        switch (g.ept) {
            case 1: return launch_fused<1, 16, SC>(a, nprob, lds, st);
            case 2: return launch_fused<2, 16, SC>(a, nprob, lds, st);
            default: return launch_fused<4, 16, SC>(a, nprob, lds, st);
        }
    }
    if (g.lpr == 4) return launch_fused<16, 4, SC>(a, nprob, lds, st);
    return g.ept == 8 ? launch_fused<8, 8, SC>(a, nprob, lds, st) : launch_fused<16, 8, SC>(a, nprob, lds, st);
}

// `nprob` (3 or 4) weighted solves, their combination AND the reverse sweep in ONE launch (one workgroup per problem):
// dC_unit [nprob,n,n] = d loss / d C at dLoss = 1 for loss = sum_p w[p] cost[p].  No dual history leaves the CU.
int kccot::sinkhorn_fused_weighted(const float* C, int nprob, const float* w, int n, float eps, int L, int Lmin,
                                   float thresh, float* cost_out, int32_t* nits_out, float* loss_out, int32_t* ticket,
                                   float* dC_unit, hipStream_t st) {
    if (!C || !cost_out || !nits_out || !loss_out || !ticket || !dC_unit || !w)
        return fail(KCCOT_EINVAL, "sinkhorn_fused: null pointer");
    if (nprob != 3 && nprob != SK_FUSED_MAXPROB) return fail(KCCOT_EINVAL, "sinkhorn_fused: nprob=%d (3 or 4)", nprob);
    if (!(eps > 0.f)) return fail(KCCOT_EINVAL, "sinkhorn_fused: eps=%g", (double)eps);
    if (!kccot_sinkhorn_fused_eligible(n, L))
        return fail(KCCOT_EUNSUPPORTED, "sinkhorn_fused: n=%d L=%d does not fit (see kccot_sinkhorn_fused_eligible)", n, L);
    const SinkGeom g = sink_geom(n, true);
    SinkFusedArgs a{C, n, L, Lmin, eps, (float)(1.0 / (double)eps), thresh, cost_out, nits_out, loss_out,
                    reinterpret_cast<int*>(ticket), dC_unit, {0.f, 0.f, 0.f, 0.f}, nullptr};
    for (int p = 0; p < nprob; ++p) a.w[p] = w[p];
#ifdef KCCOT_DIAG
    a.diag = g_fused_stamps;
#endif
    const size_t lds = fused_lds_bytes(n, L);
    return sink_shortcut_enabled() ? dispatch_fused<true>(g, a, nprob, lds, st) : dispatch_fused<false>(g, a, nprob, lds, st);
}

// The three solves of compute_sinkhorn_loss, their combination AND the reverse sweep in ONE launch:
// dC3_unit [3,n,n] = d loss / d C3 at dLoss = 1.  No dual history leaves the CU.  `ticket` as above.
extern "C" int kccot_sinkhorn_divergence_fused_f32(const float* C3, int n, float eps, int L, int Lmin, float thresh,
                                                   float* cost3_out, int32_t* nits_out, float* loss_out, int32_t* ticket,
                                                   float* dC3_unit, kccot_stream_t stream) {
    static const float w[3] = {2.0f, -1.0f, -1.0f};             // gan_utils.py:225
    if (!C3 || !cost3_out || !nits_out || !loss_out || !ticket || !dC3_unit)
        return fail(KCCOT_EINVAL, "sinkhorn_divergence_fused: null pointer");
    return sinkhorn_fused_weighted(C3, 3, w, n, eps, L, Lmin, thresh, cost3_out, nits_out, loss_out, ticket, dC3_unit,
                                   (hipStream_t)stream);
}

// Mixed Sinkhorn divergence in one launch each way (compute_sinkhorn_loss, gan_utils.py:221-225):
// the three solves of C3 = [xy, xx, yy] plus loss = 2 xy - xx - yy, combined by the last workgroup
// to finish.  `ticket` is ONE device int that must be zero on entry (the kernel leaves it zero).
extern "C" int kccot_sinkhorn_divergence_fwd_f32(const float* C3, int n, float eps, int L, int Lmin, float thresh,
                                                 float* u_hist, float* v_hist, float* cost3_out, int32_t* nits_out,
                                                 float* loss_out, int32_t* ticket, void* ws, size_t ws_bytes,
                                                 kccot_stream_t stream) {
    if (!loss_out || !ticket) return fail(KCCOT_EINVAL, "sinkhorn_divergence_fwd: null pointer");
    if (n > SK_MAXN) {   // streaming solver: no in-kernel combine; fall back to the separate launch
        int rc = kccot_sinkhorn_fwd_f32(C3, 3, n, eps, L, Lmin, thresh, KCCOT_STOP_COUNT, u_hist, v_hist, cost3_out, nits_out,
                                        nullptr, ws, ws_bytes, stream);
        if (rc) return rc;
        return kccot_mixed_divergence_fwd_f32(cost3_out, loss_out, stream);
    }
    return sinkhorn_fwd(C3, 3, n, eps, L, Lmin, thresh, KCCOT_STOP_COUNT, u_hist, v_hist, cost3_out, nits_out, nullptr, ws,
                        ws_bytes, stream, loss_out, reinterpret_cast<int*>(ticket));
}

// gloss: ONE device float dLoss/dloss; dC3_out = d loss / d C3 scaled by it.
extern "C" int kccot_sinkhorn_divergence_bwd_f32(const float* C3, const float* u_hist, const float* v_hist,
                                                 const int32_t* nits, int n, float eps, int L, const float* gloss,
                                                 float* dC3_out, void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!gloss) return fail(KCCOT_EINVAL, "sinkhorn_divergence_bwd: null pointer");
    if (n > SK_MAXN) return fail(KCCOT_EUNSUPPORTED, "sinkhorn_divergence_bwd: use mixed_divergence_bwd + sinkhorn_bwd for n > %d", SK_MAXN);
    return sinkhorn_bwd(C3, u_hist, v_hist, nits, 3, n, eps, L, gloss, dC3_out, ws, ws_bytes, stream, 1);
}

// ---- weighted marginals (include/kccot_weighted.h) ---------------------------------------------------------------------
// The solve and its reverse sweep with mu = a, nu = b instead of 1/n: an EXTENSION (the reference's compute_sinkhorn
// hard-codes the uniform marginals).  Same kernels, instantiated with the weights; the one-launch fused loss and the
// multi-CU solver are not weighted and are never selected here.
extern "C" int kccot_sinkhorn_weighted_fwd_f32(const float* C, const float* a, const float* b, int nprob, int n, float eps,
                                               int L, int Lmin, float thresh, int stop_mode, float* u_hist, float* v_hist,
                                               float* cost_out, int32_t* nits_out, float* pi_out, void* ws,
                                               size_t ws_bytes, kccot_stream_t stream) {
    if (!a || !b) return fail(KCCOT_EINVAL, "sinkhorn_weighted_fwd: null weight pointer");
    return sinkhorn_fwd(C, nprob, n, eps, L, Lmin, thresh, stop_mode, u_hist, v_hist, cost_out, nits_out, pi_out, ws,
                        ws_bytes, stream, nullptr, nullptr, a, b, 0);
}

extern "C" int kccot_sinkhorn_weighted_bwd_f32(const float* C, const float* a, const float* b, const float* u_hist,
                                               const float* v_hist, const int32_t* nits, int nprob, int n, float eps, int L,
                                               const float* gcost, float* dC_out, void* ws, size_t ws_bytes,
                                               kccot_stream_t stream) {
    if (!a || !b) return fail(KCCOT_EINVAL, "sinkhorn_weighted_bwd: null weight pointer");
    return sinkhorn_bwd(C, u_hist, v_hist, nits, nprob, n, eps, L, gcost, dC_out, ws, ws_bytes, stream, 0, a, b, 0);
}

// the same sweep, which also writes dcost/da and dcost/db [nprob,n] scaled by gcost (include/kccot_weight_grad.h)
extern "C" int kccot_sinkhorn_weighted_bwd_dw_f32(const float* C, const float* a, const float* b, const float* u_hist,
                                                  const float* v_hist, const int32_t* nits, int nprob, int n, float eps,
                                                  int L, const float* gcost, float* dC_out, float* da_out, float* db_out,
                                                  void* ws, size_t ws_bytes, kccot_stream_t stream) {
    if (!a || !b) return fail(KCCOT_EINVAL, "sinkhorn_weighted_bwd_dw: null weight pointer");
    if (!da_out || !db_out) return fail(KCCOT_EINVAL, "sinkhorn_weighted_bwd_dw: null da_out / db_out");
    return sinkhorn_bwd(C, u_hist, v_hist, nits, nprob, n, eps, L, gcost, dC_out, ws, ws_bytes, stream, 0, a, b, 0, da_out,
                        db_out);
}

// the three solves of the weighted divergence on C3 = [xy, xx, yy] with marginals (a,b), (a,a), (b,b), a = w_real,
// b = w_fake, and loss = 2 xy - xx - yy (loss.hip)
int kccot::sinkhorn_divergence_weighted_fwd(const float* C3, const float* w_real, const float* w_fake, int n, float eps,
                                            int L, int Lmin, float thresh, float* u_hist, float* v_hist, float* cost3_out,
                                            int32_t* nits_out, float* loss_out, int32_t* ticket, void* ws, size_t ws_bytes,
                                            hipStream_t st) {
    if (!w_real || !w_fake || !loss_out || !ticket) return fail(KCCOT_EINVAL, "weighted divergence: null pointer");
    if (n > SK_MAXN) {   // streaming solver: no in-kernel combine
        int rc = sinkhorn_fwd(C3, 3, n, eps, L, Lmin, thresh, KCCOT_STOP_COUNT, u_hist, v_hist, cost3_out, nits_out, nullptr,
                              ws, ws_bytes, st, nullptr, nullptr, w_real, w_fake, 1);
        if (rc) return rc;
        return kccot_mixed_divergence_fwd_f32(cost3_out, loss_out, st);
    }
    return sinkhorn_fwd(C3, 3, n, eps, L, Lmin, thresh, KCCOT_STOP_COUNT, u_hist, v_hist, cost3_out, nits_out, nullptr, ws,
                        ws_bytes, st, loss_out, reinterpret_cast<int*>(ticket), w_real, w_fake, 1);
}

// dC3 = d loss / d C3 scaled by gloss[0]; gc3: three floats of scratch (the per-problem weights, n > 128 only); da3, db3
// [3,n] (both or neither): the weight gradients of the three problems, scaled by gloss {2,-1,-1}
int kccot::sinkhorn_divergence_weighted_bwd(const float* C3, const float* w_real, const float* w_fake, const float* u_hist,
                                            const float* v_hist, const int32_t* nits, int n, float eps, int L,
                                            const float* gloss, float* gc3, float* dC3, void* ws, size_t ws_bytes,
                                            hipStream_t st, float* da3, float* db3) {
    if (!w_real || !w_fake || !gloss || !gc3) return fail(KCCOT_EINVAL, "weighted divergence backward: null pointer");
    if (n > SK_MAXN) {
        int rc = kccot_mixed_divergence_bwd_f32(gloss, gc3, st);
        if (rc) return rc;
        return sinkhorn_bwd(C3, u_hist, v_hist, nits, 3, n, eps, L, gc3, dC3, ws, ws_bytes, st, 0, w_real, w_fake, 1, da3,
                            db3);
    }
    return sinkhorn_bwd(C3, u_hist, v_hist, nits, 3, n, eps, L, gloss, dC3, ws, ws_bytes, st, 1, w_real, w_fake, 1, da3, db3);
}

// ---- conditional mode (include/kccot_conditional.h, conditional.hip) ------------------------------------------------------
// The 3 Q solves / reverse sweeps of the kernel-conditional loss on ONE shared C3 [3,n,n]: the weighted kernels with
// w_div = 2, one workgroup per problem p = 3 q + k.  No in-kernel combination (conditional.hip combines in a fixed order).
int kccot::sinkhorn_conditional_solve_fwd(const float* C3, const float* w, int Q, int n, float eps, int L, int Lmin,
                                          float thresh, float* u_hist, float* v_hist, float* cost_out, int32_t* nits_out,
                                          void* ws, size_t ws_bytes, hipStream_t st) {
    return sinkhorn_fwd(C3, 3 * Q, n, eps, L, Lmin, thresh, KCCOT_STOP_COUNT, u_hist, v_hist, cost_out, nits_out, nullptr, ws,
                        ws_bytes, st, nullptr, nullptr, w, w, 2);
}

// gcost [3 Q]: the upstream gradient of every problem's cost; dC [3 Q,n,n]: the per-problem gradients; da, db [3 Q,n] (both
// or neither): the per-problem weight gradients
int kccot::sinkhorn_conditional_solve_bwd(const float* C3, const float* w, const float* u_hist, const float* v_hist,
                                          const int32_t* nits, int Q, int n, float eps, int L, const float* gcost, float* dC,
                                          void* ws, size_t ws_bytes, hipStream_t st, float* da, float* db) {
    return sinkhorn_bwd(C3, u_hist, v_hist, nits, 3 * Q, n, eps, L, gcost, dC, ws, ws_bytes, st, 0, w, w, 2, da, db);
}
