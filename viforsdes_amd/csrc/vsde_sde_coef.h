// Drift / diffusion of the SDEs built into the library, as device functions shared by the simulator and the coefficient kernels
// (vsde_sde.hip) and the importance log-weight kernel (vsde_elbo.hip), so the closed forms exist once:
//   kind 1  Ornstein-Uhlenbeck  (examples/ornstein_uhlenbeck.py:18-30)   f = kappa (mu - x),   G = sigma
//   kind 2  Lotka-Volterra      (examples/lotka_volterra.py:18-46)       analytic 2x2 Cholesky factor, three clamp(min=1e-6)
//   kind 3  linear / diagonal   (BASELINE config 5)                       f = -a x, G = diag(softplus(b) + 1e-3)
//   kind 4  reaction network    (core/reaction_network.py)                mass action, floored Cholesky factor of sum_j h_j nu_j nu_j^T
#pragma once
#include <type_traits>

#include "vsde_common.h"

namespace vsde {

constexpr float kEmFloor = 1e-6f;
// clamp(min = 1e-6) that propagates NaN like torch.clamp / torch.maximum do (fmaxf(NaN, floor) would return the floor and hide a
// diverged path from the non-finite-loss guards of the pre-training loop and the ELBO)
__device__ __forceinline__ float floor_nan(float y) { return y < kEmFloor ? kEmFloor : y; }

constexpr int kCrnMaxS = VSDE_CRN_MAX_SPECIES, kCrnMaxR = VSDE_CRN_MAX_REACTIONS;

// state / parameter dims of the fixed-size kinds (kind 3 takes them at run time; the value here is its per-dimension slice; kind 4
// takes S and the reaction bound NR as template arguments of its kernels, R <= NR at run time: P = NR sizes its theta array)
template <int KIND> struct EmDims {
    static constexpr int S = KIND == 2 ? 2 : 1;
    static constexpr int P = KIND == 3 ? 2 : KIND == 4 ? kCrnMaxR : 3;
};

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

// ---------------------------------------------------------------------------------------------------------------------
// Kind 4: mass-action reaction network (include/vsde_hip.h: vsde_crn_network).  S is a template argument, R <= kCrnMaxR is read at
// run time.  The network travels by value in the kernel's parameter struct; every loop over reactions is unrolled to the bound
// NR (a template argument: 4, 8 or 16, the smallest that holds R) under a uniform `j < R` guard, so the tables are read at
// compile-time offsets of the kernel arguments (scalar loads) and theta_j and the per-reaction values stay in registers: an array
// indexed by a run-time j would go to scratch.  The bound keeps the table entries a small network needs, not all 16 rows, in SGPRs.
struct CrnNet {
    int R;
    int8_t order[kCrnMaxR][kCrnMaxS];   // reactant orders, 0..3
    float change[kCrnMaxR][kCrnMaxS];   // net change as float: FMA operands straight from the kernel arguments
};

// validate a C-ABI descriptor (host memory) against the call's S / P and convert it into the kernel-argument form
static inline int crn_net(const vsde_crn_network *d, int S, int P, CrnNet &n) {
    VSDE_CHECK_ARG(d, VSDE_E_BADARG, "NULL reaction-network descriptor");
    VSDE_CHECK_ARG(d->S >= 1 && d->S <= kCrnMaxS, VSDE_E_BADARG, "reaction network: %d species (1..%d supported)", d->S, kCrnMaxS);
    VSDE_CHECK_ARG(d->R >= 1 && d->R <= kCrnMaxR, VSDE_E_BADARG, "reaction network: %d reactions (1..%d supported)", d->R, kCrnMaxR);
    for (int j = 0; j < d->R; ++j)
        for (int i = 0; i < d->S; ++i)
            VSDE_CHECK_ARG(d->order[j][i] >= 0 && d->order[j][i] <= VSDE_CRN_MAX_ORDER, VSDE_E_BADARG,
                           "reaction network: reaction %d has order %d in species %d (0..%d supported)", j, (int)d->order[j][i], i,
                           VSDE_CRN_MAX_ORDER);
    VSDE_CHECK_ARG(S == d->S && P == d->R, VSDE_E_BADARG,
                   "reaction network of %d species and %d reactions called with state_dim %d, sde_param_dim %d", d->S, d->R, S, P);
    n = CrnNet{};
    n.R = d->R;
    for (int j = 0; j < d->R; ++j)
        for (int i = 0; i < d->S; ++i) { n.order[j][i] = d->order[j][i]; n.change[j][i] = (float)d->change[j][i]; }
    return 0;
}

// x^r by repeated multiplication (r uniform, 0..3) and its derivative r x^(r-1)
__device__ __forceinline__ float crn_pow(float x, int r) { return r == 0 ? 1.f : r == 1 ? x : r == 2 ? x * x : x * x * x; }
__device__ __forceinline__ float crn_dpow(float x, int r) { return r == 0 ? 0.f : r == 1 ? 1.f : r == 2 ? 2.f * x : 3.f * (x * x); }

// drift f [S] and the lower triangle of Sigma = sum_j h_j nu_j nu_j^T in sig [S][S]
template <int S, int NR>
__device__ __forceinline__ void crn_drift_cov(const CrnNet &n, const float *x, const float *th, float *f, float *sig) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        f[i] = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) sig[i * S + k] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j < n.R) {
            float m = 1.f;
#pragma unroll
            for (int i = 0; i < S; ++i) m *= crn_pow(x[i], n.order[j][i]);
            const float h = th[j] * m;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const float hn = h * n.change[j][i];
                f[i] += hn;
#pragma unroll
                for (int k = 0; k <= i; ++k) sig[i * S + k] += hn * n.change[j][k];
            }
        }
    }
}

// in place: the lower triangle of Sigma in a [S][S] -> its floored Cholesky factor (upper triangle zeroed); sd[j] = the diagonal
// quantity before its floor (the backward's clamp test)
template <int S> __device__ __forceinline__ void crn_chol(float *a, float *sd) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
        float s = a[j * S + j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= a[j * S + k] * a[j * S + k];
        sd[j] = s;
        const float ljj = sqrtf(floor_nan(s)), c = floor_nan(ljj);
        a[j * S + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < S; ++i) {
            float v = a[i * S + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= a[i * S + k] * a[j * S + k];
            a[i * S + j] = v / c;
            a[j * S + i] = 0.f;
        }
    }
}

// drift f [S] and diffusion factor G [S][S] (row-major, lower triangular) of a network at state x; th [NR]
template <int S, int NR>
__device__ __forceinline__ void crn_coef(const CrnNet &n, const float *x, const float *th, float *f, float *G) {
    float sd[S];
    crn_drift_cov<S, NR>(n, x, th, f, G);
    crn_chol<S>(G, sd);
}

// vector-Jacobian product of crn_coef: (gf [S], lower triangle of gG [S][S]) -> gx [S] (overwritten), gth [NR] (+=)
template <int S, int NR>
__device__ __forceinline__ void crn_coef_bwd(const CrnNet &n, const float *x, const float *th, const float *gf, const float *gG,
                                             float *gx, float *gth) {
    float f[S], L[S * S], sd[S], d[S * S];
    crn_drift_cov<S, NR>(n, x, th, f, L);
    crn_chol<S>(L, sd);
#pragma unroll
    for (int i = 0; i < S; ++i) {
        gx[i] = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) d[i * S + k] = gG[i * S + k];
    }
    // reverse sweep over the columns: d = adjoint of L, turned into the adjoint of Sigma column by column
#pragma unroll
    for (int j = S - 1; j >= 0; --j) {
        const float ljj = L[j * S + j], c = floor_nan(ljj);
        float dc = 0.f;
#pragma unroll
        for (int i = j + 1; i < S; ++i) {
            const float dl = d[i * S + j], da = dl / c;   // L_ij = a_ij / c:  d a_ij = dl / c,  d c -= dl L_ij / c
            dc -= da * L[i * S + j];
            d[i * S + j] = da;
#pragma unroll
            for (int k = 0; k < j; ++k) { d[i * S + k] -= da * L[j * S + k]; d[j * S + k] -= da * L[i * S + k]; }
        }
        const float dljj = d[j * S + j] + (ljj >= kEmFloor ? dc : 0.f);
        const float ds = sd[j] >= kEmFloor ? dljj / (2.f * ljj) : 0.f;
        d[j * S + j] = ds;
#pragma unroll
        for (int k = 0; k < j; ++k) d[j * S + k] -= 2.f * ds * L[j * S + k];
    }
    // through Sigma and f to the propensities, then h_j = theta_j prod_i x_i^r_ji
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j < n.R) {
            float dh = 0.f;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                float acc = gf[i];
#pragma unroll
                for (int k = 0; k <= i; ++k) acc += d[i * S + k] * n.change[j][k];
                dh += acc * n.change[j][i];
            }
            float pre[S], m = 1.f;
#pragma unroll
            for (int i = 0; i < S; ++i) { pre[i] = m; m *= crn_pow(x[i], n.order[j][i]); }
            gth[j] += dh * m;
            const float dm = dh * th[j];
            float suf = 1.f;
#pragma unroll
            for (int i = S - 1; i >= 0; --i) {
                gx[i] += dm * (pre[i] * suf) * crn_dpow(x[i], n.order[j][i]);
                suf *= crn_pow(x[i], n.order[j][i]);
            }
        }
    }
}

// y = x + f dt + (G e) sqrt(dt)
template <int S, int NR>
__device__ __forceinline__ void crn_em_step(const CrnNet &n, const float *x, const float *th, const float *e, float dt, float sqdt,
                                            float *y) {
    float f[S], G[S * S];
    crn_coef<S, NR>(n, x, th, f, G);
#pragma unroll
    for (int i = 0; i < S; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) acc += G[i * S + k] * e[k];
        y[i] = x[i] + f[i] * dt + acc * sqdt;
    }
}

// reverse-mode derivative of crn_em_step: a = dL/dy (already masked by the clamp) -> ax = dL/dx, gth += dL/dtheta
template <int S, int NR>
__device__ __forceinline__ void crn_em_step_bwd(const CrnNet &n, const float *x, const float *th, const float *e, const float *a,
                                                float dt, float sqdt, float *ax, float *gth) {
    float gf[S], gG[S * S], gx[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        gf[i] = a[i] * dt;
#pragma unroll
        for (int k = 0; k <= i; ++k) gG[i * S + k] = a[i] * e[k] * sqdt;
    }
    crn_coef_bwd<S, NR>(n, x, th, gf, gG, gx, gth);
#pragma unroll
    for (int i = 0; i < S; ++i) ax[i] = a[i] + gx[i];
}

// host: f(std::integral_constant<int, S>, std::integral_constant<int, NR>) for the run-time S in 1..kCrnMaxS and the reaction
// bound NR of R
template <int S, class F> static int crn_dispatch_r(int R, F &&f) {
    if (R <= 4) return f(std::integral_constant<int, S>{}, std::integral_constant<int, 4>{});
    if (R <= 8) return f(std::integral_constant<int, S>{}, std::integral_constant<int, 8>{});
    return f(std::integral_constant<int, S>{}, std::integral_constant<int, kCrnMaxR>{});
}
template <class F> static int crn_dispatch(int S, int R, F &&f) {
    switch (S) {
        case 1: return crn_dispatch_r<1>(R, f);
        case 2: return crn_dispatch_r<2>(R, f);
        case 3: return crn_dispatch_r<3>(R, f);
        case 4: return crn_dispatch_r<4>(R, f);
        case 5: return crn_dispatch_r<5>(R, f);
        case 6: return crn_dispatch_r<6>(R, f);
        case 7: return crn_dispatch_r<7>(R, f);
        case 8: return crn_dispatch_r<8>(R, f);
        default: set_error("reaction network: %d species (1..%d supported)", S, kCrnMaxS); return VSDE_E_BADARG;
    }
}

}  // namespace vsde
