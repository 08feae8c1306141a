// What smooth.hip, smooth_sigma.hip and smooth_aniso.hip share: the host-side taps of the Gaussian stencils and the two-pass form of the
// max-normalisation adjoint's batch sums.  (What the two tile walks of smooth_sigma.hip and smooth_aniso.hip share beyond that --
// the tiling rule, the geometry of a plan, REFLECT, the combine kernel -- is in tile_walk.h.)
#pragma once
#include "common.h"
#include <math.h>
#include <stdint.h>

namespace kccot {

constexpr int SM_MAXR = 7;

struct Taps { float w[2 * SM_MAXR + 1]; int r; };

// data_utils.py:483-491: kernel = exp(-0.5/sigma^2 * x^2) (fp32), normalised by its fp32 sum
static Taps make_taps(float sigma, int r) {
    Taps tp{};
    tp.r = r;
    const float coef = (float)(-0.5 / ((double)sigma * (double)sigma));
    float sum = 0.f;
    for (int d = -r; d <= r; ++d) { tp.w[d + r] = expf(coef * (float)(d * d)); sum += tp.w[d + r]; }
    for (int d = 0; d <= 2 * r; ++d) tp.w[d] /= sum;
    return tp;
}

// KCCOT_SMOOTH_CAUSAL_T (NOT reference behaviour: the reference has no one-sided smoothing).  w[d] = exp(-d^2 / (2 sigma^2)),
// d = 0..r, is the non-negative half of the taps above before their normalisation (w[0] = 1); iz[t] = 1 / Z_t with
// Z_t = w[0] + .. + w[min(r, t)] summed in fp32 in ascending d, t = 0..r (every t >= r has Z_r).  Entries behind r are zero.
struct CausalTaps { float w[SM_MAXR + 1]; float iz[SM_MAXR + 1]; int r; };

static CausalTaps make_causal_taps(float sigma, int r) {
    CausalTaps ct{};
    ct.r = r;
    const float coef = (float)(-0.5 / ((double)sigma * (double)sigma));
    float z = 0.f;
    for (int d = 0; d <= r; ++d) { ct.w[d] = expf(coef * (float)(d * d)); z += ct.w[d]; ct.iz[d] = 1.0f / z; }
    return ct;
}

// The derivative taps of include/kccot_smooth_sigma.h (shared by smooth_sigma.hip and smooth_aniso.hip).
// symmetric axis: w = the forward's taps (make_taps), dw[d + r] = w_d (d^2 - mu2) / sigma^3
struct SymD { float w[2 * SM_MAXR + 1]; float dw[2 * SM_MAXR + 1]; };
// causal T: row min(t, r) holds v_{t,d} = w_d / Z_t and its derivative for d = 0..r; zero behind d = min(t, r)
struct CausD { float v[SM_MAXR + 1][SM_MAXR + 1]; float dv[SM_MAXR + 1][SM_MAXR + 1]; };

// fp64 from the fp32 value of sigma, rounded to fp32 at the end
static SymD make_sym_d(float sigma, int r) {
    SymD s{};
    const Taps tp = make_taps(sigma, r);
    const double sg = (double)sigma;
    double e[2 * SM_MAXR + 1], z = 0.0, mu2 = 0.0;
    for (int d = -r; d <= r; ++d) { e[d + r] = exp(-(double)(d * d) / (2.0 * sg * sg)); z += e[d + r]; }
    for (int d = -r; d <= r; ++d) mu2 += e[d + r] / z * (double)(d * d);
    for (int d = -r; d <= r; ++d) {
        s.w[d + r] = tp.w[d + r];
        s.dw[d + r] = (float)(e[d + r] / z * ((double)(d * d) - mu2) / (sg * sg * sg));
    }
    return s;
}

static CausD make_caus_d(float sigma, int r) {
    CausD c{};
    const CausalTaps ct = make_causal_taps(sigma, r);
    const double sg = (double)sigma;
    for (int t = 0; t <= r; ++t) {
        double e[SM_MAXR + 1], z = 0.0, mu2 = 0.0;
        for (int d = 0; d <= t; ++d) { e[d] = exp(-(double)(d * d) / (2.0 * sg * sg)); z += e[d]; }
        for (int d = 0; d <= t; ++d) mu2 += e[d] / z * (double)(d * d);
        for (int d = 0; d <= t; ++d) {
            c.v[t][d] = ct.w[d] * ct.iz[t];
            c.dv[t][d] = (float)(e[d] / z * ((double)(d * d) - mu2) / (sg * sg * sg));
        }
    }
    return c;
}

// res[0..1] = {sum(gout * out), #(out == 1)} over n elements in two launches (smooth.hip): pdot and pcnt hold
// (n + 255) / 256 floats each.  The form KCCOT_SMOOTH_STATS_ONLY runs; every caller gets the same bits from the same data.
int smooth_maxnorm_stats(const float* gout, const float* out, int64_t n, float* pdot, float* pcnt, float* res, hipStream_t st);

}  // namespace kccot
