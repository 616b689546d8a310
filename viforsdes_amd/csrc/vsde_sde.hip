// Batched Euler-Maruyama simulator of the MODEL SDE and its reverse-mode gradient (gfx950).
// Replaces the T-step Python loop of the reference's core/euler_maruyama.py:11-45 (two user callbacks, an einsum, an
// in-place clamp and a slice-assign per step: ~10 tiny kernels x T) for the SDEs whose drift / diffusion are built in:
//   kind 1  Ornstein-Uhlenbeck  (examples/ornstein_uhlenbeck.py:18-30)   f = kappa (mu - x),   G = sigma
//   kind 2  Lotka-Volterra      (examples/lotka_volterra.py:18-46)       analytic 2x2 Cholesky factor, three clamp(min=1e-6)
//   kind 3  linear / diagonal   (BASELINE config 5)                       f = -a x, G = diag(softplus(b) + 1e-3)
//   kind 4  reaction network    (core/reaction_network.py)                S species (template, <= 8), R <= 16 reactions
// One thread per sample path, the time loop inside the kernel, x_t in registers.  HBM-bound streaming (noise read once,
// trajectory written once; the backward reads noise, trajectory and the upstream gradient once): a path's records are
// contiguous over time, so the 64 paths of a workgroup move CH steps at a time through LDS as coalesced row segments.
// The backward is what torch autograd computes for trainer.py:208-259 (pre-training differentiates the simulation with
// respect to theta): reverse recursion over the saved trajectory, a clamped entry (== 1e-6) passes no gradient.
#include "vsde_sde_step.h"

namespace vsde {

constexpr int kEmPaths = 64;   // paths per workgroup (one wavefront)
constexpr int kEmChunk = 32;   // time steps staged per LDS round (S <= 2)
// steps per LDS round at S dims: the backward stages three [64][(CH+1) S + 1] float buffers, 53 KiB at S = 4 and 56 KiB at S = 8
constexpr int em_chunk(int S) { return S <= 2 ? kEmChunk : S <= 4 ? 16 : 8; }

struct EmParams {
    int B, T, S, P;
    const float *x0, *theta, *noise, *traj_in, *g_traj;
    float *traj, *g_x0, *g_theta;
    uint32_t pos_mask;
    float dt, sqdt;
    CrnNet net;    // kind 4
};

// reverse-mode derivative of em_step: a = dL/dy (already masked by the clamp) -> ax = dL/dx, gth += dL/dtheta
template <int KIND>
__device__ __forceinline__ void em_step_bwd(const float *x, const float *th, const float *e, const float *a, float dt,
                                            float sqdt, float *ax, float *gth) {
    if constexpr (KIND == 1) {
        gth[0] += a[0] * (th[1] - x[0]) * dt; gth[1] += a[0] * th[0] * dt; gth[2] += a[0] * e[0] * sqdt;
        ax[0] = a[0] * (1.f - th[0] * dt);
    } else if constexpr (KIND == 2) {
        const float u = x[0], v = x[1], t1 = th[0], t2 = th[1], t3 = th[2], uv = t2 * u * v;
        const float q00r = t1 * u + uv, l00 = sqrtf(floor_nan(q00r));
        const float c = floor_nan(l00), l10 = -uv / c;
        const float q11r = t3 * v + uv - l10 * l10, l11 = sqrtf(floor_nan(q11r));
        const float d_f0 = a[0] * dt, d_f1 = a[1] * dt, d_l11 = a[1] * e[1] * sqdt;
        float d_l00 = a[0] * e[0] * sqdt, d_l10 = a[1] * e[0] * sqdt;
        float d_u = a[0], d_v = a[1], d_uv = 0.f, d_t1 = 0.f, d_t3 = 0.f;
        const float d_q11 = q11r >= kEmFloor ? d_l11 / (2.f * l11) : 0.f;
        d_t3 += d_q11 * v; d_v += d_q11 * t3; d_uv += d_q11; d_l10 += -2.f * l10 * d_q11;
        d_uv += -d_l10 / c;
        if (l00 >= kEmFloor) d_l00 += d_l10 * uv / (c * c);
        const float d_q00 = q00r >= kEmFloor ? d_l00 / (2.f * l00) : 0.f;
        d_t1 += d_q00 * u; d_u += d_q00 * t1; d_uv += d_q00;
        d_t1 += d_f0 * u; d_u += d_f0 * t1; d_uv -= d_f0;
        d_uv += d_f1; d_t3 -= d_f1 * v; d_v -= d_f1 * t3;
        gth[0] += d_t1; gth[1] += d_uv * u * v; gth[2] += d_t3;
        ax[0] = d_u + d_uv * t2 * v; ax[1] = d_v + d_uv * t2 * u;
    } else {
        const float b = th[1];
        gth[0] += a[0] * (-x[0]) * dt;
        gth[1] += a[0] * (b > 20.f ? 1.f : fast_rcp(1.f + __expf(-b))) * e[0] * sqdt;
        ax[0] = a[0] * (1.f - th[0] * dt);
    }
}

// Move `count` floats of each of the workgroup's 64 path rows between global memory (row r at g + r*gstride) and LDS
// (row r at s + r*sstride): each wave instruction covers one contiguous run of a single row.
template <bool LOAD>
__device__ __forceinline__ void em_rows(float *s, int sstride, float *g, int64_t gstride, int count, int rows, int lane) {
    for (int r = 0; r < rows; ++r)
        for (int k = lane; k < count; k += kEmPaths) {
            if constexpr (LOAD) s[r * sstride + k] = g[(int64_t)r * gstride + k];
            else g[(int64_t)r * gstride + k] = s[r * sstride + k];
        }
}

// kinds 1, 2, 4: thread = path
template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false>
__global__ void __launch_bounds__(kEmPaths) em_fwd_kernel(EmParams p) {
    constexpr int S = NS, P = KIN ? 2 * NR : NR, CH = em_chunk(S), RS = CH * S + 1;
    __shared__ float noise_s[kEmPaths * RS], traj_s[kEmPaths * RS];
    const int lane = threadIdx.x, b0 = blockIdx.x * kEmPaths, b = b0 + lane;
    const int rows = min(kEmPaths, p.B - b0);
    const bool valid = b < p.B;
    float x[S], th[P];
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = valid ? p.x0[(int64_t)b * S + i] : 1.f;
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, p.net.R, valid);
    else em_load_theta<KIND, P>(th, p.theta, b, p.P, valid);
    if (valid)
#pragma unroll
        for (int i = 0; i < S; ++i) p.traj[(int64_t)b * (p.T + 1) * S + i] = x[i];
    for (int t0 = 0; t0 < p.T; t0 += CH) {
        const int n = min(CH, p.T - t0);
        em_rows<true>(noise_s, RS, const_cast<float *>(p.noise) + ((int64_t)b0 * p.T + t0) * S, (int64_t)p.T * S, n * S, rows, lane);
        __syncthreads();
        for (int k = 0; k < n; ++k) {
            float y[S];
            if constexpr (KIND == 4) crn_em_step<S, NR, KIN>(p.net, x, th, noise_s + lane * RS + k * S, p.dt, p.sqdt, y);
            else em_step<KIND>(x, th, noise_s + lane * RS + k * S, p.dt, p.sqdt, y);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                x[i] = ((p.pos_mask >> i) & 1u) ? floor_nan(y[i]) : y[i];
                traj_s[lane * RS + k * S + i] = x[i];
            }
        }
        __syncthreads();
        em_rows<false>(traj_s, RS, p.traj + ((int64_t)b0 * (p.T + 1) + t0 + 1) * S, (int64_t)(p.T + 1) * S, n * S, rows, lane);
        __syncthreads();
    }
}

template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false>
__global__ void __launch_bounds__(kEmPaths) em_bwd_kernel(EmParams p) {
    constexpr int S = NS, P = KIN ? 2 * NR : NR, CH = em_chunk(S), RS = (CH + 1) * S + 1;
    __shared__ float noise_s[kEmPaths * RS], traj_s[kEmPaths * RS], g_s[kEmPaths * RS];
    const int lane = threadIdx.x, b0 = blockIdx.x * kEmPaths, b = b0 + lane;
    const int rows = min(kEmPaths, p.B - b0);
    const bool valid = b < p.B;
    float a[S], th[P], gth[P];
#pragma unroll
    for (int i = 0; i < S; ++i) a[i] = 0.f;
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, p.net.R, valid);
    else em_load_theta<KIND, P>(th, p.theta, b, p.P, valid);
#pragma unroll
    for (int k = 0; k < P; ++k) gth[k] = 0.f;
    const int nchunks = (p.T + CH - 1) / CH;
    for (int c = nchunks - 1; c >= 0; --c) {
        const int t0 = c * CH, n = min(CH, p.T - t0);
        em_rows<true>(noise_s, RS, const_cast<float *>(p.noise) + ((int64_t)b0 * p.T + t0) * S, (int64_t)p.T * S, n * S, rows, lane);
        em_rows<true>(traj_s, RS, const_cast<float *>(p.traj_in) + ((int64_t)b0 * (p.T + 1) + t0) * S, (int64_t)(p.T + 1) * S,
                      (n + 1) * S, rows, lane);                                             // x_{t0} .. x_{t0+n}
        em_rows<true>(g_s, RS, const_cast<float *>(p.g_traj) + ((int64_t)b0 * (p.T + 1) + t0 + 1) * S, (int64_t)(p.T + 1) * S,
                      n * S, rows, lane);                                                   // upstream of x_{t0+1} .. x_{t0+n}
        __syncthreads();
        for (int k = n - 1; k >= 0; --k) {
            const float *xs = traj_s + lane * RS + k * S;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                a[i] += g_s[lane * RS + k * S + i];
                if (((p.pos_mask >> i) & 1u) && xs[S + i] == kEmFloor) a[i] = 0.f;          // clamped entry: no gradient
            }
            float ax[S];
            if constexpr (KIND == 4) crn_em_step_bwd<S, NR, KIN>(p.net, xs, th, noise_s + lane * RS + k * S, a, p.dt, p.sqdt, ax, gth);
            else em_step_bwd<KIND>(xs, th, noise_s + lane * RS + k * S, a, p.dt, p.sqdt, ax, gth);
#pragma unroll
            for (int i = 0; i < S; ++i) a[i] = ax[i];
        }
        __syncthreads();
    }
    if (valid) {
#pragma unroll
        for (int i = 0; i < S; ++i) p.g_x0[(int64_t)b * S + i] = a[i] + p.g_traj[(int64_t)b * (p.T + 1) * S + i];
        if constexpr (KIN) {
            crn_store_rates<NR>(p.g_theta, gth, b, p.net.R);
        } else {
            const int np = KIND == 4 ? p.P : P;
#pragma unroll
            for (int k = 0; k < P; ++k)
                if (k < np) p.g_theta[(int64_t)b * np + k] = gth[k];
        }
    }
}

// kind 3: every state dimension is an independent scalar SDE -> thread = (path, dim); neighbouring threads are neighbouring
// addresses at every step, so the accesses coalesce without staging
__global__ void __launch_bounds__(256) em_diag_fwd_kernel(EmParams p) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)p.B * p.S) return;
    const int b = (int)(q / p.S), i = (int)(q % p.S);
    const float th[2] = {p.theta[(int64_t)b * p.P + i], p.theta[(int64_t)b * p.P + p.S + i]};
    const bool pos = (p.pos_mask >> i) & 1u;
    float x = p.x0[q];
    float *tr = p.traj + (int64_t)b * (p.T + 1) * p.S + i;
    const float *nz = p.noise + (int64_t)b * p.T * p.S + i;
    tr[0] = x;
    for (int t = 0; t < p.T; ++t) {
        float y;
        em_step<3>(&x, th, nz + (int64_t)t * p.S, p.dt, p.sqdt, &y);
        x = pos ? floor_nan(y) : y;
        tr[(int64_t)(t + 1) * p.S] = x;
    }
}

__global__ void __launch_bounds__(256) em_diag_bwd_kernel(EmParams p) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (int64_t)p.B * p.S) return;
    const int b = (int)(q / p.S), i = (int)(q % p.S);
    const float th[2] = {p.theta[(int64_t)b * p.P + i], p.theta[(int64_t)b * p.P + p.S + i]};
    const bool pos = (p.pos_mask >> i) & 1u;
    const float *tr = p.traj_in + (int64_t)b * (p.T + 1) * p.S + i, *gt = p.g_traj + (int64_t)b * (p.T + 1) * p.S + i;
    const float *nz = p.noise + (int64_t)b * p.T * p.S + i;
    float a = 0.f, gth[2] = {0.f, 0.f};
    for (int t = p.T - 1; t >= 0; --t) {
        a += gt[(int64_t)(t + 1) * p.S];
        if (pos && tr[(int64_t)(t + 1) * p.S] == kEmFloor) a = 0.f;
        float ax;
        em_step_bwd<3>(tr + (int64_t)t * p.S, th, nz + (int64_t)t * p.S, &a, p.dt, p.sqdt, &ax, gth);
        a = ax;
    }
    p.g_x0[q] = a + gt[0];
    p.g_theta[(int64_t)b * p.P + i] = gth[0];
    p.g_theta[(int64_t)b * p.P + p.S + i] = gth[1];
}

// ---------------------------------------------------------------------------------------------------------------------
// Forecast: the recursion of em_fwd_kernel / em_diag_fwd_kernel run for T steps from x_start with its Gaussian increments made
// in the kernel, keeping only the states at K requested steps.  Neither the noise nor the trajectory exists in memory.
// Noise stream (include/vsde_hip.h): the normal of (path b, step t, dim i) is number t % 4 of
// philox4x32_10(counter {t / 4, i, b, 0}, key {key[0], key[1]}) through Box-Muller on the word pairs (w0, w1), (w2, w3)
// (vsde_sde_step.h: fc_normals).
struct FcParams {
    int B, T, S, P, K;
    const float *x0, *theta;
    const int *steps;
    const uint32_t *key;
    float *out;
    uint32_t pos_mask;
    float dt, sqdt;
    CrnNet net;    // kind 4
};

// kinds 1, 2, 4: thread = path (all S dims per thread); kind 3: thread = (path, dim), one dim per thread.  A block of 4 steps
// is branch-free: the Philox / Box-Muller work of the NEXT block depends on no state, so it sits in the same basic block as the
// 4-step serial chain and the scheduler interleaves the two.  Output rows are written after the block from the 4 kept states
// (out_steps is the same for every thread: the write loop is uniform).  Steps that never come (out_steps above T) read NaN.
template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false>
__global__ void __launch_bounds__(256) forecast_kernel(FcParams p) {
    constexpr int S = NS, P = KIN ? 2 * NR : NR;
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int b, d0, rs;                          // path, first state dim of this thread, row stride of x_start / out
    if constexpr (KIND == 3) {
        if (q >= (int64_t)p.B * p.S) return;
        b = (int)(q / p.S); d0 = (int)(q % p.S); rs = p.S;
    } else {
        if (q >= p.B) return;
        b = (int)q; d0 = 0; rs = S;
    }
    const uint32_t k0 = p.key[0], k1 = p.key[1];
    float x[S], th[P];
    bool pos[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        x[i] = p.x0[(int64_t)b * rs + d0 + i];
        pos[i] = (p.pos_mask >> (d0 + i)) & 1u;
    }
    if constexpr (KIND == 3) {
        th[0] = p.theta[(int64_t)b * p.P + d0]; th[1] = p.theta[(int64_t)b * p.P + p.S + d0];
    } else if constexpr (KIN) {
        crn_load_rates<NR>(th, p.theta, b, p.net.R, true);
    } else {
        em_load_theta<KIND, P>(th, p.theta, b, p.P, true);
    }
    float *o = p.out + (int64_t)b * p.K * rs + d0;
    int k = 0, next = p.steps[0];
    float zn[S][4];
#pragma unroll
    for (int i = 0; i < S; ++i) fc_normals(0u, (uint32_t)(d0 + i), (uint32_t)b, k0, k1, zn[i]);
    const int nblk = (p.T + 3) / 4;
    for (int blk = 0; blk < nblk && k < p.K; ++blk) {
        float z[S][4], xs[4][S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
#pragma unroll
            for (int j = 0; j < 4; ++j) z[i][j] = zn[i][j];
            fc_normals((uint32_t)(blk + 1), (uint32_t)(d0 + i), (uint32_t)b, k0, k1, zn[i]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float e[S], y[S];
#pragma unroll
            for (int i = 0; i < S; ++i) e[i] = z[i][j];
            if constexpr (KIND == 4) crn_em_step<S, NR, KIN>(p.net, x, th, e, p.dt, p.sqdt, y);
            else em_step<KIND>(x, th, e, p.dt, p.sqdt, y);
#pragma unroll
            for (int i = 0; i < S; ++i) xs[j][i] = x[i] = pos[i] ? floor_nan(y[i]) : y[i];
            if constexpr (KIND == 4) {
                // kind 4 writes its rows as the states are made: at S = 8 the [4][S] staging would push the kernel into scratch
                const int t = 4 * blk + j + 1;
                while (k < p.K && next <= t && t <= p.T) {
#pragma unroll
                    for (int i = 0; i < S; ++i) o[(int64_t)k * rs + i] = x[i];
                    if (++k < p.K) next = p.steps[k];
                }
            }
        }
        // steps past T in the last block are computed and never written: rows are written for out_steps <= t1 only
        const int t1 = min(4 * blk + 4, p.T);
        while (KIND != 4 && k < p.K && next <= t1) {
            const int j = max(next - 4 * blk - 1, 0);
#pragma unroll
            for (int i = 0; i < S; ++i)
                o[(int64_t)k * rs + i] = j == 0 ? xs[0][i] : j == 1 ? xs[1][i] : j == 2 ? xs[2][i] : xs[3][i];
            if (++k < p.K) next = p.steps[k];
        }
    }
    for (; k < p.K; ++k)
#pragma unroll
        for (int i = 0; i < S; ++i) o[(int64_t)k * rs + i] = __builtin_nanf("");
}

// ---------------------------------------------------------------------------------------------------------------------
// Drift f(x_t, theta) and diffusion factor G(x_t, theta) of the built-in SDEs on every grid point of a batch of paths, and
// the vector-Jacobian product the ELBO backward needs.  Replaces the ~35 (forward) + ~70 (autograd backward) tiny torch
// kernels the Python drift / diffusion callables expand to on the flattened [(B T), S] states
// (inference/evidence_lower_bound.py:37-40 of the reference evaluates them exactly there).
//   x [B][T+1][S] (rows 0..T-1 used), theta [B][P]  ->  drift [B][T][S], diffusion [B][T][S][S]
//   backward: g_drift, g_diff -> g_x [B][T+1][S] (row T = 0), g_theta [B][P] (sum over t, fixed order)
// torch.clamp(min=1e-6) passes the gradient where the input is >= the bound.
struct CoefParams {
    int B, T, S, P;
    const float *x, *theta, *g_drift, *g_diff;
    float *drift, *diff, *g_x, *g_theta;
    CrnNet net;    // kind 4
};

// coef_fwd<KIND> (vsde_sde_coef.h) and its vector-Jacobian product
template <int KIND>
__device__ __forceinline__ void coef_bwd(const float *x, const float *th, const float *gf, const float *gG, float *gx, float *gth) {
    if constexpr (KIND == 1) {
        gth[0] += gf[0] * (th[1] - x[0]); gth[1] += gf[0] * th[0]; gth[2] += gG[0];
        gx[0] = -gf[0] * th[0];
    } else {
        const float u = x[0], v = x[1], t1 = th[0], t2 = th[1], t3 = th[2], uv = t2 * u * v;
        const float q00r = t1 * u + uv, l00 = sqrtf(floor_nan(q00r));
        const float c = floor_nan(l00), l10 = -uv / c;
        const float q11r = t3 * v + uv - l10 * l10, l11 = sqrtf(floor_nan(q11r));
        float d_l00 = gG[0], d_l10 = gG[2];
        float d_u = 0.f, d_v = 0.f, d_uv = 0.f, d_t1 = 0.f, d_t3 = 0.f;
        const float d_q11 = q11r >= kEmFloor ? gG[3] / (2.f * l11) : 0.f;
        d_t3 += d_q11 * v; d_v += d_q11 * t3; d_uv += d_q11; d_l10 += -2.f * l10 * d_q11;
        d_uv += -d_l10 / c;
        if (l00 >= kEmFloor) d_l00 += d_l10 * uv / (c * c);
        const float d_q00 = q00r >= kEmFloor ? d_l00 / (2.f * l00) : 0.f;
        d_t1 += d_q00 * u; d_u += d_q00 * t1; d_uv += d_q00;
        d_t1 += gf[0] * u; d_u += gf[0] * t1; d_uv -= gf[0];
        d_uv += gf[1]; d_t3 -= gf[1] * v; d_v -= gf[1] * t3;
        gth[0] += d_t1; gth[1] += d_uv * u * v; gth[2] += d_t3;
        gx[0] = d_u + d_uv * t2 * v; gx[1] = d_v + d_uv * t2 * u;
    }
}

// thread = grid point (b, t)
template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false>
__global__ void __launch_bounds__(256) coef_fwd_kernel(CoefParams p) {
    constexpr int S = NS, P = KIN ? 2 * NR : NR;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)p.B * p.T) return;
    const int b = (int)(q / p.T), t = (int)(q % p.T);
    float x[S], th[P], f[S], G[S * S];
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = p.x[((int64_t)b * (p.T + 1) + t) * S + i];
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, p.net.R, true);
    else em_load_theta<KIND, P>(th, p.theta, b, p.P, true);
    if constexpr (KIND == 4) crn_coef<S, NR, KIN>(p.net, x, th, f, G);
    else coef_fwd<KIND>(x, th, f, G);
#pragma unroll
    for (int i = 0; i < S; ++i) p.drift[q * S + i] = f[i];
#pragma unroll
    for (int i = 0; i < S * S; ++i) p.diff[q * S * S + i] = G[i];
}

// workgroup = path: threads walk the time steps, the theta gradient is reduced through LDS in a fixed tree
template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false>
__global__ void __launch_bounds__(256) coef_bwd_kernel(CoefParams p) {
    constexpr int S = NS, P = KIN ? 2 * NR : NR;
    __shared__ float red[256][P + 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    float th[P], gth[P];
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, p.net.R, true);
    else em_load_theta<KIND, P>(th, p.theta, b, p.P, true);
#pragma unroll
    for (int i = 0; i < P; ++i) gth[i] = 0.f;
    for (int t = tid; t <= p.T; t += 256) {
        float gx[S];
        if (t < p.T) {
            const int64_t q = (int64_t)b * p.T + t;
            float x[S], gf[S], gG[S * S];
#pragma unroll
            for (int i = 0; i < S; ++i) { x[i] = p.x[((int64_t)b * (p.T + 1) + t) * S + i]; gf[i] = p.g_drift[q * S + i]; }
#pragma unroll
            for (int i = 0; i < S * S; ++i) gG[i] = p.g_diff[q * S * S + i];
            if constexpr (KIND == 4) crn_coef_bwd<S, NR, KIN>(p.net, x, th, gf, gG, gx, gth);
            else coef_bwd<KIND>(x, th, gf, gG, gx, gth);
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) gx[i] = 0.f;
        }
#pragma unroll
        for (int i = 0; i < S; ++i) p.g_x[((int64_t)b * (p.T + 1) + t) * S + i] = gx[i];
    }
#pragma unroll
    for (int i = 0; i < P; ++i) red[tid][i] = gth[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int i = 0; i < P; ++i) red[tid][i] += red[tid + w][i];
        __syncthreads();
    }
    if constexpr (KIN) {
        const int R = p.net.R;          // red[0] holds (k_0 .. k_{NR-1}, K_0 .. K_{NR-1}); g_theta [B][2R]
        if (tid < 2 * R) p.g_theta[(int64_t)b * 2 * R + tid] = red[0][tid < R ? tid : NR + tid - R];
    } else {
        const int np = KIND == 4 ? p.P : P;
        if (tid < np) p.g_theta[(int64_t)b * np + tid] = red[0][tid];
    }
}

// kind 3 (f_i = -a_i x_i, G = diag(softplus(b_i) + 1e-3)): thread = (b, t, i) forward; workgroup = path backward with the threads
// laid out as (time slot, i)
__global__ void __launch_bounds__(256) coef_diag_fwd_kernel(CoefParams p) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= (int64_t)p.B * p.T * p.S) return;
    const int i = (int)(q % p.S);
    const int64_t bt = q / p.S;
    const int b = (int)(bt / p.T), t = (int)(bt % p.T);
    const float a = p.theta[(int64_t)b * p.P + i], g = softplus_f(p.theta[(int64_t)b * p.P + p.S + i]) + 1e-3f;
    p.drift[q] = -a * p.x[((int64_t)b * (p.T + 1) + t) * p.S + i];
    float *row = p.diff + q * p.S;
    for (int j = 0; j < p.S; ++j) row[j] = j == i ? g : 0.f;
}

__global__ void __launch_bounds__(256) coef_diag_bwd_kernel(CoefParams p) {
    __shared__ float red[256][2];
    const int b = blockIdx.x, tid = threadIdx.x, S = p.S;
    const int slots = 256 / S, slot = tid / S, i = tid % S;
    float ga = 0.f, gb = 0.f;
    if (slot < slots) {
        const float a = p.theta[(int64_t)b * p.P + i];
        for (int t = slot; t <= p.T; t += slots) {
            float gx = 0.f;
            if (t < p.T) {
                const int64_t q = ((int64_t)b * p.T + t) * S + i;
                const float gf = p.g_drift[q];
                gx = -gf * a;
                ga -= gf * p.x[((int64_t)b * (p.T + 1) + t) * S + i];
                gb += p.g_diff[q * S + i];
            }
            p.g_x[((int64_t)b * (p.T + 1) + t) * S + i] = gx;
        }
    }
    red[tid][0] = ga; red[tid][1] = gb;
    __syncthreads();
    if (tid < S) {
        float sa = 0.f, sb = 0.f;
        for (int k = 0; k < slots; ++k) { sa += red[k * S + tid][0]; sb += red[k * S + tid][1]; }
        const float bb = p.theta[(int64_t)b * p.P + S + tid];
        p.g_theta[(int64_t)b * p.P + tid] = sa;
        p.g_theta[(int64_t)b * p.P + S + tid] = sb * (bb > 20.f ? 1.f : 1.f / (1.f + expf(-bb)));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host: one body per operation, taking the model route (vsde_sde_coef.h: SdeRoute); the exported functions below build the route
// and forward.  Every check, the descriptor's included, comes before the first HIP call.

// the checks the five operations share (what: the operation, for the message) and the dims of its parameter block
template <class Params> static int sde_begin(Params &p, const SdeRoute &rt, const char *what, int B, int T, int S, int P) {
    const int rc = route_check(rt, S, P, p.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(rt.kind != 3 || (S >= 1 && S <= 32), VSDE_E_BADARG, "linear-diagonal SDE needs state_dim 1..32 (got %d)", S);
    VSDE_CHECK_ARG(B > 0 && T > 0, VSDE_E_BADARG, "bad %s dims B=%d T=%d", what, B, T);
    p.B = B; p.T = T; p.S = S; p.P = P;
    return 0;
}

template <class Params> static void sde_time(Params &p, double time_step, const uint8_t *positive_mask_host) {
    p.pos_mask = em_mask(positive_mask_host, p.S); p.dt = (float)time_step; p.sqdt = (float)sqrt(time_step);
}

template <class Kern, class Params> static int sde_launch(Kern kern, dim3 grid, dim3 block, const Params &p, void *stream) {
    hipLaunchKernelGGL(kern, grid, block, 0, (hipStream_t)stream, p);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

// the simulators' geometry: a 64-thread workgroup of paths, or (kind 3) a thread per (path, dim)
template <int KIND> static dim3 em_grid(int B, int S) {
    return KIND == 3 ? dim3((unsigned)(((int64_t)B * S + 255) / 256)) : dim3((B + kEmPaths - 1) / kEmPaths);
}
template <int KIND> static dim3 em_block() { return KIND == 3 ? dim3(256) : dim3(kEmPaths); }

static int em_fwd(const SdeRoute &rt, int B, int T, int S, int P, const float *x0, const float *theta, const float *noise,
                  double time_step, const uint8_t *positive_mask_host, float *traj, void *stream) {
    EmParams p = {};
    const int rc = sde_begin(p, rt, "Euler-Maruyama", B, T, S, P);
    if (rc) return rc;
    VSDE_CHECK_ARG(x0 && theta && noise && traj && time_step > 0, VSDE_E_BADARG, "NULL argument / bad time_step");
    p.x0 = x0; p.theta = theta; p.noise = noise; p.traj = traj;
    sde_time(p, time_step, positive_mask_host);
    return route_dispatch<0>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
        constexpr int KIND = decltype(kind)::value;
        if constexpr (KIND == 3) return sde_launch(em_diag_fwd_kernel, em_grid<3>(B, S), em_block<3>(), p, stream);
        else return sde_launch(em_fwd_kernel<KIND, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>, em_grid<KIND>(B, S),
                               em_block<KIND>(), p, stream);
    });
}

static int em_bwd(const SdeRoute &rt, int B, int T, int S, int P, const float *theta, const float *noise, const float *traj,
                  const float *g_traj, double time_step, const uint8_t *positive_mask_host, float *g_x0, float *g_theta,
                  void *stream) {
    EmParams p = {};
    const int rc = sde_begin(p, rt, "Euler-Maruyama", B, T, S, P);
    if (rc) return rc;
    VSDE_CHECK_ARG(theta && noise && traj && g_traj && g_x0 && g_theta && time_step > 0, VSDE_E_BADARG, "NULL argument / bad time_step");
    p.theta = theta; p.noise = noise; p.traj_in = traj; p.g_traj = g_traj; p.g_x0 = g_x0; p.g_theta = g_theta;
    sde_time(p, time_step, positive_mask_host);
    return route_dispatch<0>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
        constexpr int KIND = decltype(kind)::value;
        if constexpr (KIND == 3) return sde_launch(em_diag_bwd_kernel, em_grid<3>(B, S), em_block<3>(), p, stream);
        else return sde_launch(em_bwd_kernel<KIND, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>, em_grid<KIND>(B, S),
                               em_block<KIND>(), p, stream);
    });
}

static int forecast(const SdeRoute &rt, int B, int T, int S, int P, int K, const float *x_start, const float *theta,
                    const int *out_steps, const uint32_t *key, double time_step, const uint8_t *positive_mask_host, float *out,
                    void *stream) {
    FcParams p = {};
    const int rc = sde_begin(p, rt, "forecast", B, T, S, P);
    if (rc) return rc;
    VSDE_CHECK_ARG(K > 0, VSDE_E_BADARG, "bad forecast output count K=%d", K);
    VSDE_CHECK_ARG(x_start && theta && out_steps && key && out && time_step > 0, VSDE_E_BADARG, "NULL argument / bad time_step");
    p.K = K; p.x0 = x_start; p.theta = theta; p.steps = out_steps; p.key = key; p.out = out;
    sde_time(p, time_step, positive_mask_host);
    return route_dispatch<0>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
        constexpr int KIND = decltype(kind)::value;
        return sde_launch(forecast_kernel<KIND, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>, em_grid<KIND>(B, S),
                          em_block<KIND>(), p, stream);
    });
}

static int coefficients_fwd(const SdeRoute &rt, int B, int T, int S, int P, const float *x, const float *theta, float *drift,
                            float *diffusion, void *stream) {
    CoefParams p = {};
    const int rc = sde_begin(p, rt, "coefficient", B, T, S, P);
    if (rc) return rc;
    VSDE_CHECK_ARG(x && theta && drift && diffusion, VSDE_E_BADARG, "NULL argument");
    p.x = x; p.theta = theta; p.drift = drift; p.diff = diffusion;
    // a thread per (path, step), or (kind 3) per (path, step, dim)
    return route_dispatch<0>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
        constexpr int KIND = decltype(kind)::value;
        const dim3 grid((unsigned)(((int64_t)B * T * (KIND == 3 ? S : 1) + 255) / 256));
        if constexpr (KIND == 3) return sde_launch(coef_diag_fwd_kernel, grid, dim3(256), p, stream);
        else return sde_launch(coef_fwd_kernel<KIND, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>, grid, dim3(256), p,
                               stream);
    });
}

static int coefficients_bwd(const SdeRoute &rt, int B, int T, int S, int P, const float *x, const float *theta, const float *g_drift,
                            const float *g_diffusion, float *g_x, float *g_theta, void *stream) {
    CoefParams p = {};
    const int rc = sde_begin(p, rt, "coefficient", B, T, S, P);
    if (rc) return rc;
    VSDE_CHECK_ARG(x && theta && g_drift && g_diffusion && g_x && g_theta, VSDE_E_BADARG, "NULL argument");
    p.x = x; p.theta = theta; p.g_drift = g_drift; p.g_diff = g_diffusion; p.g_x = g_x; p.g_theta = g_theta;
    return route_dispatch<0>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
        constexpr int KIND = decltype(kind)::value;
        if constexpr (KIND == 3) return sde_launch(coef_diag_bwd_kernel, dim3(B), dim3(256), p, stream);
        else return sde_launch(coef_bwd_kernel<KIND, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>, dim3(B), dim3(256), p,
                               stream);
    });
}

}  // namespace vsde

using namespace vsde;

// Built-in kinds 1..3
extern "C" int vsde_euler_maruyama_fwd(int kind, int B, int T, int S, int P, const float *x0, const float *theta,
                                       const float *noise, double time_step, const uint8_t *positive_mask_host, float *traj,
                                       void *stream) {
    return em_fwd(SdeRoute{kind}, B, T, S, P, x0, theta, noise, time_step, positive_mask_host, traj, stream);
}

extern "C" int vsde_euler_maruyama_bwd(int kind, int B, int T, int S, int P, const float *theta, const float *noise,
                                       const float *traj, const float *g_traj, double time_step,
                                       const uint8_t *positive_mask_host, float *g_x0, float *g_theta, void *stream) {
    return em_bwd(SdeRoute{kind}, B, T, S, P, theta, noise, traj, g_traj, time_step, positive_mask_host, g_x0, g_theta, stream);
}

extern "C" int vsde_forecast(int kind, int B, int T, int S, int P, int K, const float *x_start, const float *theta,
                             const int *out_steps, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                             float *out, void *stream) {
    return forecast(SdeRoute{kind}, B, T, S, P, K, x_start, theta, out_steps, key, time_step, positive_mask_host, out, stream);
}

extern "C" int vsde_sde_coefficients_fwd(int kind, int B, int T, int S, int P, const float *x, const float *theta, float *drift,
                                         float *diffusion, void *stream) {
    return coefficients_fwd(SdeRoute{kind}, B, T, S, P, x, theta, drift, diffusion, stream);
}

extern "C" int vsde_sde_coefficients_bwd(int kind, int B, int T, int S, int P, const float *x, const float *theta,
                                         const float *g_drift, const float *g_diffusion, float *g_x, float *g_theta, void *stream) {
    return coefficients_bwd(SdeRoute{kind}, B, T, S, P, x, theta, g_drift, g_diffusion, g_x, g_theta, stream);
}

// Kind 4: reaction networks (include/vsde_hip.h: vsde_crn_network), theta [B][R]
extern "C" int vsde_crn_euler_maruyama_fwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *x0,
                                           const float *theta, const float *noise, double time_step,
                                           const uint8_t *positive_mask_host, float *traj, void *stream) {
    return em_fwd(crn_route(net), B, T, S, P, x0, theta, noise, time_step, positive_mask_host, traj, stream);
}

extern "C" int vsde_crn_euler_maruyama_bwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *theta,
                                           const float *noise, const float *traj, const float *g_traj, double time_step,
                                           const uint8_t *positive_mask_host, float *g_x0, float *g_theta, void *stream) {
    return em_bwd(crn_route(net), B, T, S, P, theta, noise, traj, g_traj, time_step, positive_mask_host, g_x0, g_theta, stream);
}

extern "C" int vsde_crn_forecast(const vsde_crn_network *net, int B, int T, int S, int P, int K, const float *x_start,
                                 const float *theta, const int *out_steps, const uint32_t *key, double time_step,
                                 const uint8_t *positive_mask_host, float *out, void *stream) {
    return forecast(crn_route(net), B, T, S, P, K, x_start, theta, out_steps, key, time_step, positive_mask_host, out, stream);
}

extern "C" int vsde_crn_sde_coefficients_fwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *x,
                                             const float *theta, float *drift, float *diffusion, void *stream) {
    return coefficients_fwd(crn_route(net), B, T, S, P, x, theta, drift, diffusion, stream);
}

extern "C" int vsde_crn_sde_coefficients_bwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *x,
                                             const float *theta, const float *g_drift, const float *g_diffusion, float *g_x,
                                             float *g_theta, void *stream) {
    return coefficients_bwd(crn_route(net), B, T, S, P, x, theta, g_drift, g_diffusion, g_x, g_theta, stream);
}

// Kind 4 with rate laws (include/vsde_hip.h: vsde_crn_kinetics): the KIN instantiations, theta = the effective constants
// rates [B][2R]
extern "C" int vsde_crn_kinetic_euler_maruyama_fwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S,
                                                   int P, const float *x0, const float *rates, const float *noise,
                                                   double time_step, const uint8_t *positive_mask_host, float *traj,
                                                   void *stream) {
    return em_fwd(crn_route(net, kin), B, T, S, P, x0, rates, noise, time_step, positive_mask_host, traj, stream);
}

extern "C" int vsde_crn_kinetic_euler_maruyama_bwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S,
                                                   int P, const float *rates, const float *noise, const float *traj,
                                                   const float *g_traj, double time_step, const uint8_t *positive_mask_host,
                                                   float *g_x0, float *g_rates, void *stream) {
    return em_bwd(crn_route(net, kin), B, T, S, P, rates, noise, traj, g_traj, time_step, positive_mask_host, g_x0, g_rates,
                  stream);
}

extern "C" int vsde_crn_kinetic_forecast(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int P,
                                         int K, const float *x_start, const float *rates, const int *out_steps,
                                         const uint32_t *key, double time_step, const uint8_t *positive_mask_host, float *out,
                                         void *stream) {
    return forecast(crn_route(net, kin), B, T, S, P, K, x_start, rates, out_steps, key, time_step, positive_mask_host, out,
                    stream);
}

extern "C" int vsde_crn_kinetic_sde_coefficients_fwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T,
                                                     int S, int P, const float *x, const float *rates, float *drift,
                                                     float *diffusion, void *stream) {
    return coefficients_fwd(crn_route(net, kin), B, T, S, P, x, rates, drift, diffusion, stream);
}

extern "C" int vsde_crn_kinetic_sde_coefficients_bwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T,
                                                     int S, int P, const float *x, const float *rates, const float *g_drift,
                                                     const float *g_diffusion, float *g_x, float *g_rates, void *stream) {
    return coefficients_bwd(crn_route(net, kin), B, T, S, P, x, rates, g_drift, g_diffusion, g_x, g_rates, stream);
}
