// What smooth.hip and smooth_sigma.hip share: the host-side taps of the Gaussian stencils and the two-pass form of the
// max-normalisation adjoint's batch sums.
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

// res[0..1] = {sum(gout * out), #(out == 1)} over n elements in two launches (smooth.hip): pdot and pcnt hold
// (n + 255) / 256 floats each.  The form KCCOT_SMOOTH_STATS_ONLY runs; every caller gets the same bits from the same data.
int smooth_maxnorm_stats(const float* gout, const float* out, int64_t n, float* pdot, float* pcnt, float* res, hipStream_t st);

}  // namespace kccot
