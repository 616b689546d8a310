// One Euler-Maruyama step of the built-in SDEs and the specified Philox4x32-10 / Box-Muller noise stream, as device functions
// shared by the simulator and forecast kernels (vsde_sde.hip) and the particle filter (vsde_filter.hip), so both exist once.
#pragma once
#include "vsde_sde_coef.h"

namespace vsde {

// y = x + f dt + (G eps) sqrt(dt)
template <int KIND>
__device__ __forceinline__ void em_step(const float *x, const float *th, const float *e, float dt, float sqdt, float *y) {
    if constexpr (KIND == 1) {
        y[0] = x[0] + th[0] * (th[1] - x[0]) * dt + th[2] * e[0] * sqdt;
    } else if constexpr (KIND == 2) {
        const float u = x[0], v = x[1], uv = th[1] * u * v;
        const float l00 = sqrtf(floor_nan(th[0] * u + uv));
        const float l10 = -uv / floor_nan(l00);
        const float l11 = sqrtf(floor_nan(th[2] * v + uv - l10 * l10));
        y[0] = u + (th[0] * u - uv) * dt + (l00 * e[0]) * sqdt;
        y[1] = v + (uv - th[2] * v) * dt + (l10 * e[0] + l11 * e[1]) * sqdt;
    } else {
        y[0] = x[0] + (-th[0] * x[0]) * dt + ((softplus_f(th[1]) + 1e-3f) * e[0]) * sqdt;
    }
}

// row b of theta [B][np] into th [P] (kind 4: np = R <= P at run time, the rest 1)
template <int KIND, int P>
__device__ __forceinline__ void em_load_theta(float *th, const float *theta, int b, int np, bool valid) {
    if constexpr (KIND != 4) np = P;
#pragma unroll
    for (int k = 0; k < P; ++k) th[k] = (valid && k < np) ? theta[(int64_t)b * np + k] : 1.f;
}

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c;
}

// u = ((w >> 8) + 0.5) 2^-24 in (0, 1] (fp32, round to nearest even)
__device__ __forceinline__ float philox_uniform(uint32_t w) { return ((float)(w >> 8) + 0.5f) * 5.9604644775390625e-8f; }

// r = sqrt(-2 ln u_a): |z| <= sqrt(50 ln 2) ~ 5.89
__device__ __forceinline__ void box_muller(uint32_t wa, uint32_t wb, float &za, float &zb) {
    const float ua = ((float)(wa >> 8) + 0.5f) * 5.9604644775390625e-8f, ub = ((float)(wb >> 8) + 0.5f) * 5.9604644775390625e-8f;
    const float r = sqrtf(-2.f * logf(ua));
    float s, c;
    sincospif(2.f * ub, &s, &c);
    za = r * c; zb = r * s;
}

// normals of steps 4 blk .. 4 blk + 3 of (path b, dim i)
__device__ __forceinline__ void fc_normals(uint32_t blk, uint32_t i, uint32_t b, uint32_t k0, uint32_t k1, float *z) {
    const uint4 w = philox4x32_10(make_uint4(blk, i, b, 0u), k0, k1);
    box_muller(w.x, w.y, z[0], z[1]);
    box_muller(w.z, w.w, z[2], z[3]);
}

// host: S bytes -> the kernels' bit mask of the positive state dims
static inline uint32_t em_mask(const uint8_t *m, int S) {
    uint32_t r = 0;
    for (int i = 0; i < S && m; ++i) r |= (m[i] ? 1u : 0u) << i;
    return r;
}

}  // namespace vsde
