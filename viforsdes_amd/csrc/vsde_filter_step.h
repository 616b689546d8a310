// What the particle-filter translation units share (gfx950): the limits and the argument block of the filter kernels, the
// propagation of one particle between two observations (pf_propagate: Euler-Maruyama; pf_propagate_guided: the modified-diffusion-
// bridge step of the guided filter, and with RES its residual form) with a store hook, and the host helpers that fill the
// argument block.  vsde_filter_kernels.h builds the three kernels on it (the filter, the replay of its genealogy, the replay of
// carried path records), so they run one step code.
#pragma once
#include "vsde_sde_step.h"

namespace vsde {

constexpr int kPfMaxN = 1024, kPfWaves = kPfMaxN / kWave, kPfMaxS = 16, kPfMaxO = 16;
constexpr int kPfRed = kPfWaves * (kPfMaxS + 2);   // floats of the reduction stage
constexpr int kPfResidualFullS = 3;   // the largest state dim whose residual-bridge instantiations fit a 1024-thread workgroup

// Particles per filter an instantiation is built for.  A 1024-thread workgroup leaves 128 VGPRs per lane; the reaction-network step
// at 5..8 species (its S x S covariance and Cholesky factor in registers) needs more, so those instantiations are built for 512
// threads (256 VGPRs) and refuse a larger N rather than spill.
// The guided step (A, psi, W, C and their factors next to f and G) fits the 128 VGPRs up to S = 3 (at most 122); at S = 4 it
// would spill (12..68 bytes of scratch per lane), so the guided S = 4 instantiations are 512-thread ones too.
// The residual variant of the guided step carries eta and eta_end, and f(eta) within a step (3 S floats), on top of that: up to
// S = kPfResidualFullS it still fits (at most 127), so today its rule is the guided one; the argument keeps the two apart.
constexpr int pf_max_n(int kind, int S, bool guided = false, bool residual = false) {
    return (kind == 4 && S > 4) || (guided && S > 3) || (residual && S > kPfResidualFullS) ? kPfMaxN / 2 : kPfMaxN;
}

constexpr int kPfGuidedMaxS = 4, kPfGuidedMaxO = 4;
constexpr float kPfPivotFloor = 1e-6f;   // inference/particle_filter.py: BRIDGE_PIVOT_FLOOR

struct PfParams {
    int M, N, S, P, K, O;
    const float *x0, *theta, *obs_values, *obs_matrix;
    const int *rows;
    const uint32_t *key;
    float *loglik, *incr, *ess, *mean, *std, *particles;
    int *ancestors;
    uint32_t pos_mask;
    float dt, sqdt, inv_var, log_norm, log_n;
    CrnNet net;    // kind 4
    // guided variant only (at the end: the bootstrap kernels read their arguments at the offsets they always had)
    float var;
    float *log_weights;
    // count observation term (CNT instantiations only)
    CountLik cl;
};

// Store hook of pf_propagate / pf_propagate_guided: st(t, i, v) sees dim i of the state after grid step t.  The filter keeps no
// trajectory: its hook is empty, so its instantiations are the code they were; the replay kernel (rp_kernel) stores the state
struct PfNoStore {
    __device__ __forceinline__ void operator()(int, int, float) const {}
};

// Euler-Maruyama steps t0 .. t1 - 1 (global grid steps, t1 > t0) of one particle, path index b of the noise stream
template <int KIND, int NS, int NR, bool KIN, int P, class ST = PfNoStore>
__device__ __forceinline__ void pf_propagate(const PfParams &p, float *x, const float *th, int t0, int t1, uint32_t b, uint32_t k0,
                                             uint32_t k1, int m, ST st = ST()) {
    if constexpr (KIND == 3) {
        // independent scalar SDEs: one dim at a time, so only 4 normals are alive (theta_i is uniform: scalar loads)
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            {
                const float th2[2] = {p.theta[(int64_t)m * p.P + i], p.theta[(int64_t)m * p.P + NS + i]};
                const bool pos = (p.pos_mask >> i) & 1u;
                float xi = x[i];
                for (int blk = t0 >> 2; blk <= (t1 - 1) >> 2; ++blk) {
                    float z[4];
                    fc_normals((uint32_t)blk, (uint32_t)i, b, k0, k1, z);
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int t = 4 * blk + q;
                        if (t >= t0 && t < t1) {
                            float y;
                            em_step<3>(&xi, th2, &z[q], p.dt, p.sqdt, &y);
                            xi = pos ? floor_nan(y) : y;
                            st(t, i, xi);
                        }
                    }
                }
                x[i] = xi;
            }
        }
    } else {
        for (int blk = t0 >> 2; blk <= (t1 - 1) >> 2; ++blk) {
            float z[NS][4];
#pragma unroll
            for (int i = 0; i < NS; ++i) fc_normals((uint32_t)blk, (uint32_t)i, b, k0, k1, z[i]);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int t = 4 * blk + q;
                if (t >= t0 && t < t1) {
                    float e[NS], y[NS];
#pragma unroll
                    for (int i = 0; i < NS; ++i) e[i] = z[i][q];
                    if constexpr (KIND == 4) crn_em_step<NS, NR, KIN>(p.net, x, th, e, p.dt, p.sqdt, y);
                    else em_step<KIND>(x, th, e, p.dt, p.sqdt, y);
#pragma unroll
                    for (int i = 0; i < NS; ++i) x[i] = ((p.pos_mask >> i) & 1u) ? floor_nan(y[i]) : y[i];
#pragma unroll
                    for (int i = 0; i < NS; ++i) st(t, i, x[i]);
                }
            }
        }
    }
}

// in place: the lower triangle of a [N][N] -> its Cholesky factor; FLOOR: every pivot is floored at kPfPivotFloor before its square
// root (NaN stays NaN).  inv[j] = 1 / L_jj
template <int N, bool FLOOR> __device__ __forceinline__ void pf_chol(float *a, float *inv) {
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float s = a[j * N + j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= a[j * N + k] * a[j * N + k];
        if constexpr (FLOOR) s = s < kPfPivotFloor ? kPfPivotFloor : s;
        const float d = sqrtf(s);
        a[j * N + j] = d;
        inv[j] = 1.f / d;
#pragma unroll
        for (int i = j + 1; i < N; ++i) {
            float v = a[i * N + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= a[i * N + k] * a[j * N + k];
            a[i * N + j] = v * inv[j];
        }
    }
}

// the drift alone, f(x) [NS] (the residual bridge's deterministic path): the coefficient functions with the diffusion factor left to
// the compiler to drop
template <int KIND, int NS, int NR, bool KIN>
__device__ __forceinline__ void pf_drift(const PfParams &p, const float *x, const float *th, float *f) {
    if constexpr (KIND == 3) {
#pragma unroll
        for (int i = 0; i < NS; ++i) f[i] = -th[i] * x[i];
    } else {
        [[maybe_unused]] float G[NS * NS];
        if constexpr (KIND == 4) crn_drift_cov<NS, NR, KIN>(p.net, x, th, f, G);
        else coef_fwd<KIND>(x, th, f, G);
    }
}

// eta <- clamp(eta + dt f): one noise-free Euler step with the state's own clamp
template <int NS> __device__ __forceinline__ void pf_ode_step(const PfParams &p, float *eta, const float *f) {
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        const float y = eta[i] + f[i] * p.dt;
        eta[i] = ((p.pos_mask >> i) & 1u) ? floor_nan(y) : y;
    }
}

// One guided Euler step (modified diffusion bridge) of a particle at x towards the observation yk that is nleft grid steps ahead:
// A = sqrt(dt) H G, psi = nleft A A^T + var I = R R^T, W = R^-1 A, r = R^-1 (yk - H (x + nleft dt f)), m = W^T r, C = I - W^T W =
// M M^T (floored pivots), eps = m + M z, x <- clamp(x + f dt + sqrt(dt) G eps), lr += -|eps|^2 / 2 + |z|^2 / 2 + sum log M_jj.
// Rows o >= O of A, psi and the residual are exact zeros (psi_oo = var), so they add nothing.  th: kinds 1, 2, 4 as em_load_theta /
// crn_load_rates leave it; kind 3: th[i] = a_i, th[NS + i] = softplus(b_i) + 1e-3
// RES (the residual bridge): the predicted endpoint x + nleft dt f is replaced by eta_end + (x - eta) + nleft dt (f - f(eta)) with
// eta the noise-free Euler path from the segment's start state and eta_end its end at the observation's row; eta then takes its
// own step with the f(eta) already formed.  Everything else is the same code.
template <int KIND, int NS, int NR, bool KIN, int NO, bool RES = false>
__device__ __forceinline__ void pf_bridge_step(const PfParams &p, float *x, const float *th, const float *z, const float *yk,
                                               float nleft, float &lr, [[maybe_unused]] float *eta = nullptr,
                                               [[maybe_unused]] const float *eta_end = nullptr) {
    float f[NS], G[NS * NS];
    if constexpr (KIND == 4) {
        crn_coef<NS, NR, KIN>(p.net, x, th, f, G);
    } else if constexpr (KIND == 3) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            f[i] = -th[i] * x[i];
#pragma unroll
            for (int k = 0; k < NS; ++k) G[i * NS + k] = i == k ? th[NS + i] : 0.f;
        }
    } else {
        coef_fwd<KIND>(x, th, f, G);
    }
    const float ndt = nleft * p.dt;
    [[maybe_unused]] float ahead[NS];   // RES: the predicted state at the observation's row
    if constexpr (RES) {
        float fe[NS];
        pf_drift<KIND, NS, NR, KIN>(p, eta, th, fe);
#pragma unroll
        for (int i = 0; i < NS; ++i) ahead[i] = eta_end[i] + (x[i] - eta[i]) + ndt * (f[i] - fe[i]);
        pf_ode_step<NS>(p, eta, fe);
    }
    float A[NO * NS], e[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o) {
#pragma unroll
        for (int i = 0; i < NS; ++i) A[o * NS + i] = 0.f;
        e[o] = 0.f;
        if (o < p.O) {
            float pred = 0.f;
            if (p.obs_matrix) {
#pragma unroll
                for (int k = 0; k < NS; ++k) {
                    const float h = p.obs_matrix[o * NS + k];
                    if constexpr (RES) pred += h * ahead[k];
                    else pred += h * (x[k] + ndt * f[k]);
#pragma unroll
                    for (int i = 0; i <= k; ++i) A[o * NS + i] += h * G[k * NS + i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < NS; ++i)
                    if (i <= o && o < NS) A[o * NS + i] = G[(o < NS ? o : 0) * NS + i];
                if constexpr (RES) pred = ahead[o < NS ? o : 0];
                else pred = x[o < NS ? o : 0] + ndt * f[o < NS ? o : 0];
            }
#pragma unroll
            for (int i = 0; i < NS; ++i) A[o * NS + i] *= p.sqdt;
            e[o] = yk[o] - pred;
        }
    }
    float psi[NO * NO], rinv[NO];
#pragma unroll
    for (int o = 0; o < NO; ++o)
#pragma unroll
        for (int q = 0; q <= o; ++q) {
            float acc = 0.f;
#pragma unroll
            for (int i = 0; i < NS; ++i) acc += A[o * NS + i] * A[q * NS + i];
            psi[o * NO + q] = nleft * acc + (o == q ? p.var : 0.f);
        }
    pf_chol<NO, false>(psi, rinv);
    // forward substitution, in place: A <- W = R^-1 A, e <- r = R^-1 e
#pragma unroll
    for (int o = 0; o < NO; ++o) {
#pragma unroll
        for (int q = 0; q < o; ++q) {
#pragma unroll
            for (int i = 0; i < NS; ++i) A[o * NS + i] -= psi[o * NO + q] * A[q * NS + i];
            e[o] -= psi[o * NO + q] * e[q];
        }
#pragma unroll
        for (int i = 0; i < NS; ++i) A[o * NS + i] *= rinv[o];
        e[o] *= rinv[o];
    }
    float C[NS * NS], minv[NS], eps[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        float mi = 0.f;
#pragma unroll
        for (int o = 0; o < NO; ++o) mi += A[o * NS + i] * e[o];
        eps[i] = mi;
#pragma unroll
        for (int k = 0; k <= i; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int o = 0; o < NO; ++o) acc += A[o * NS + i] * A[o * NS + k];
            C[i * NS + k] = (i == k ? 1.f : 0.f) - acc;
        }
    }
    pf_chol<NS, true>(C, minv);
    float dl = 0.f;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
#pragma unroll
        for (int k = 0; k <= i; ++k) eps[i] += C[i * NS + k] * z[k];
        dl += -0.5f * eps[i] * eps[i] + 0.5f * z[i] * z[i] + logf(C[i * NS + i]);
    }
    lr += dl;
#pragma unroll
    for (int i = 0; i < NS; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) acc += G[i * NS + k] * eps[k];
        const float y = x[i] + f[i] * p.dt + acc * p.sqdt;
        f[i] = ((p.pos_mask >> i) & 1u) ? floor_nan(y) : y;
    }
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = f[i];
}

// guided steps t0 .. t1 - 1 of one particle towards the observation yk at grid row t1.  RES: the segment opens with the noise-free
// Euler pass from x over its t1 - t0 steps (drift only), whose end eta_end and running state eta stay in registers
template <int KIND, int NS, int NR, bool KIN, int NO, bool RES = false, class ST = PfNoStore>
__device__ __forceinline__ void pf_propagate_guided(const PfParams &p, float *x, const float *th, int t0, int t1, uint32_t b,
                                                    uint32_t k0, uint32_t k1, const float *yk, float &lr, ST st = ST()) {
    [[maybe_unused]] float eta[NS], eta_end[NS];
    if constexpr (RES) {
#pragma unroll
        for (int i = 0; i < NS; ++i) eta[i] = eta_end[i] = x[i];
        for (int t = t0; t < t1; ++t) {
            float fe[NS];
            pf_drift<KIND, NS, NR, KIN>(p, eta_end, th, fe);
            pf_ode_step<NS>(p, eta_end, fe);
        }
    }
    for (int blk = t0 >> 2; blk <= (t1 - 1) >> 2; ++blk) {
        float z[NS][4];
#pragma unroll
        for (int i = 0; i < NS; ++i) fc_normals((uint32_t)blk, (uint32_t)i, b, k0, k1, z[i]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = 4 * blk + q;
            if (t >= t0 && t < t1) {
                float zq[NS];
#pragma unroll
                for (int i = 0; i < NS; ++i) zq[i] = z[i][q];
                if constexpr (RES) pf_bridge_step<KIND, NS, NR, KIN, NO, true>(p, x, th, zq, yk, (float)(t1 - t), lr, eta, eta_end);
                else pf_bridge_step<KIND, NS, NR, KIN, NO>(p, x, th, zq, yk, (float)(t1 - t), lr);
#pragma unroll
                for (int i = 0; i < NS; ++i) st(t, i, x[i]);
            }
        }
    }
}

// the Gaussian observation model: the filter's weights and the bridge proposal; the count entry points pass variance 1
static inline int pf_obs(PfParams &p, int S, int O, const float *obs_values, const float *obs_matrix, double variance) {
    VSDE_CHECK_ARG(obs_matrix || O == S, VSDE_E_BADARG, "without an observation matrix obs_dim must equal state_dim (%d vs %d)", O, S);
    VSDE_CHECK_ARG(variance > 0, VSDE_E_BADARG, "bad variance / time_step");
    p.obs_values = obs_values; p.obs_matrix = obs_matrix; p.var = (float)variance;
    p.inv_var = (float)(1.0 / variance); p.log_norm = (float)(-0.5 * log(2.0 * M_PI * variance));
    return 0;
}

// what the filter and the replay read alike
static inline void pf_fill(PfParams &p, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta, const int *obs_rows,
                    const uint32_t *key, double time_step, const uint8_t *positive_mask_host) {
    p.M = M; p.N = N; p.S = S; p.P = P; p.K = K; p.O = O; p.x0 = x0; p.theta = theta; p.rows = obs_rows; p.key = key;
    p.pos_mask = em_mask(positive_mask_host, S); p.dt = (float)time_step; p.sqdt = (float)sqrt(time_step);
}

// the replay kernels: a thread is not tied to a particle, 256-thread workgroups (512 VGPRs a lane) keep every instantiation out of scratch
constexpr int kRpThreads = 256;

// the state after grid step t goes to row t + 1 of the draw's path [T + 1][S]
struct RpStore {
    float *path;
    int S;
    __device__ __forceinline__ void operator()(int t, int i, float v) const { path[(int64_t)(t + 1) * S + i] = v; }
};

}  // namespace vsde
