// A Poisson draw on the counter-based Philox stream, as a device function (gfx950): the sampler of the tau-leap kernels
// (vsde_tau_leap.hip).  viforsdes_amd/core/tau_leap.py (poisson_draw) is the specification.
//
// Everything runs in float64; only lam carries the caller's precision.  The accept test of PTRS subtracts terms of size n log lam
// (1e5 at lam = 1e4) to get an O(1) result: in fp32 it decides about a percent of the attempts wrongly.  A tau-leap step costs R
// draws, not events, and most attempts are accepted by the squeeze before log and lgamma are reached.
//
//   lam == 0: 0, no words read.
//   lam < 10: inversion by sequential search on u1 of attempt 0: p = F = exp(-lam), n = 0; while u1 > F and n < 63: n += 1,
//             p = p (lam / n), F = F + p.  (U can be exactly 1.0, hence the bound.)
//   lam >= 10: Hoermann's PTRS (1993): b = 0.931 + 2.53 sqrt(lam), a = -0.059 + 0.02483 b, 1/alpha = 1.1239 + 1.1328 / (b - 3.4),
//             v_r = 0.9277 - 3.6224 / (b - 2).  Attempt q: Uc = u1 - 0.5, V = u2, us = 0.5 - |Uc|; reject if us < 0.013 and V > us
//             (first: us can be 0); n = floor(((2 a) / us + b) Uc + lam + 0.43); accept if us >= 0.07 and V <= v_r; reject if
//             n < 0; accept if (log V + log(1/alpha)) - log(a / (us us) + b) <= (-lam + n log lam) - lgamma(n + 1).  At most 32
//             attempts; the draw fails (-1) after the 32nd.
// Attempt q of reaction j at step t of path b reads w = philox4x32_10({t, j | ((q >> 1) << 16), b, 8}, key): u1 = U(w[2 (q & 1)]),
// u2 = U(w[2 (q & 1) + 1]), U(w) = ((w >> 8) + 0.5) 2^-24 in fp32.
//
// The products and sums below are the specification's, one rounding each: contraction into FMAs is switched off in this function.
#pragma once
#include "vsde_sde_step.h"

namespace vsde {

constexpr uint32_t kPoissonStreamWord = 8u;   // fourth counter word; 0..7 are taken (core/jump_process.py lists them)
constexpr int kPoissonMaxAttempts = 32, kPoissonInversionMax = 63;
constexpr double kPoissonInversionBelow = 10.0;

// lgamma(n + 1) for an integer-valued n >= 0: the argument is shifted up to z >= 16 by the recurrence (lgamma(z) = lgamma(z + 1)
// - log z: one log of an exact product of at most 15 factors), then Stirling's series through the z^-9 term, whose remainder is
// below 691 / (360360 z^11) < 1.1e-16 there.  The library's general lgamma (poles, reflection, several ranges) costs this kernel
// some 100 VGPRs it has no use for.
__device__ __forceinline__ double poisson_lgamma1p(double n) {
    double z = n + 1.0, prod = 1.0;
#pragma unroll 1
    while (z < 16.0) { prod *= z; z += 1.0; }
    const double r = 1.0 / z, r2 = r * r;
    const double series = r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0)))));
    return ((z - 0.5) * log(z) - z + 0.91893853320467274178) + series - log(prod);
}

// n >= 0, or -1 when the 32nd PTRS attempt was rejected.  lam: finite, >= 0, at most 2^30 (the accepted n then fits an int)
__device__ __forceinline__ int poisson_draw(double lam, uint32_t t, uint32_t j, uint32_t b, uint32_t k0, uint32_t k1) {
#pragma clang fp contract(off)
    if (!(lam > 0.0)) return 0;
    uint4 w = philox4x32_10(make_uint4(t, j, b, kPoissonStreamWord), k0, k1);
    if (lam < kPoissonInversionBelow) {
        const double u1 = (double)philox_uniform(w.x);
        double p = exp(-lam), F = p;
        int n = 0;
        while (u1 > F && n < kPoissonInversionMax) {
            ++n;
            p = p * (lam / (double)n);
            F = F + p;
        }
        return n;
    }
    const double bb = 0.931 + 2.53 * sqrt(lam), a = -0.059 + 0.02483 * bb;
    const double inv_alpha = 1.1239 + 1.1328 / (bb - 3.4), v_r = 0.9277 - 3.6224 / (bb - 2.0);
    const double log_lam = log(lam), log_inv_alpha = log(inv_alpha);
#pragma unroll 1
    for (int q = 0; q < kPoissonMaxAttempts; ++q) {
        if (q != 0 && (q & 1) == 0) w = philox4x32_10(make_uint4(t, j | ((uint32_t)(q >> 1) << 16), b, kPoissonStreamWord), k0, k1);
        const double u1 = (double)philox_uniform((q & 1) ? w.z : w.x), V = (double)philox_uniform((q & 1) ? w.w : w.y);
        const double Uc = u1 - 0.5, us = 0.5 - fabs(Uc);
        if (us < 0.013 && V > us) continue;
        const double n = floor(((2.0 * a) / us + bb) * Uc + lam + 0.43);
        if (us >= 0.07 && V <= v_r) return (int)n;
        if (n < 0.0) continue;
        const double lhs = (log(V) + log_inv_alpha) - log(a / (us * us) + bb);
        const double rhs = (-lam + n * log_lam) - poisson_lgamma1p(n);
        if (lhs <= rhs) return (int)n;
    }
    return -1;
}

}  // namespace vsde
