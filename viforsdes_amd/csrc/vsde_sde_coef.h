// Drift / diffusion of the SDEs built into the library, as device functions shared by the simulator and the coefficient kernels
// (vsde_sde.hip) and the importance log-weight kernel (vsde_elbo.hip), so the closed forms exist once:
//   kind 1  Ornstein-Uhlenbeck  (examples/ornstein_uhlenbeck.py:18-30)   f = kappa (mu - x),   G = sigma
//   kind 2  Lotka-Volterra      (examples/lotka_volterra.py:18-46)       analytic 2x2 Cholesky factor, three clamp(min=1e-6)
//   kind 3  linear / diagonal   (BASELINE config 5)                       f = -a x, G = diag(softplus(b) + 1e-3)
#pragma once
#include "vsde_common.h"

namespace vsde {

constexpr float kEmFloor = 1e-6f;
// clamp(min = 1e-6) that propagates NaN like torch.clamp / torch.maximum do (fmaxf(NaN, floor) would return the floor and hide a
// diverged path from the non-finite-loss guards of the pre-training loop and the ELBO)
__device__ __forceinline__ float floor_nan(float y) { return y < kEmFloor ? kEmFloor : y; }

// state / parameter dims of the fixed-size kinds (kind 3 takes them at run time; the value here is its per-dimension slice)
template <int KIND> struct EmDims { static constexpr int S = KIND == 2 ? 2 : 1; static constexpr int P = KIND == 3 ? 2 : 3; };

// F.softplus (threshold 20)
__device__ __forceinline__ float softplus_f(float b) { return b > 20.f ? b : log1pf(__expf(b)); }

// drift f [S] and diffusion factor G [S][S] (row-major, lower triangular) of kinds 1, 2 at state x
template <int KIND> __device__ __forceinline__ void coef_fwd(const float *x, const float *th, float *f, float *G) {
    if constexpr (KIND == 1) {
        f[0] = th[0] * (th[1] - x[0]); G[0] = th[2];
    } else {
        const float u = x[0], v = x[1], uv = th[1] * u * v;
        const float l00 = sqrtf(floor_nan(th[0] * u + uv));
        const float l10 = -uv / floor_nan(l00);
        const float l11 = sqrtf(floor_nan(th[2] * v + uv - l10 * l10));
        f[0] = th[0] * u - uv; f[1] = uv - th[2] * v;
        G[0] = l00; G[1] = 0.f; G[2] = l10; G[3] = l11;
    }
}

}  // namespace vsde
