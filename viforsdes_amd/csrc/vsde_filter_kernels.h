// The three kernels that run the particle filter's step code (gfx950) and the host body of each operation: pf_kernel (the filter),
// rp_kernel (the replay of its genealogy) and ar_kernel (the replay of carried path records).  Templates only: vsde_filter.hip and
// vsde_anchored.hip instantiate the bootstrap and bridge forms behind their entry points, vsde_residual.hip the residual-bridge
// forms (template argument RES) of all three, so the translation units compile side by side.
#pragma once
#include "vsde_filter_step.h"

namespace vsde {

__device__ __forceinline__ float pf_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

// v[0 .. NV) summed over the workgroup, the result in every thread: butterfly per wave (every lane adds the same pairs, so the lanes
// agree bitwise), wave totals through red [nwaves][NV], added in wave order
template <int NV>
__device__ __forceinline__ void pf_block_sum(float *v, float *red, int lane, int wave, int nwaves) {
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < NV; ++i) red[wave * NV + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float s = 0.f;
        for (int w = 0; w < nwaves; ++w) s += red[w * NV + i];
        v[i] = s;
    }
    __syncthreads();
}

// workgroup = filter m (theta_m), thread = particle j.  NS: the state dim (kind 3: one instantiation per dim: a run-time dim under
// `i < S` guards costs a hoisted 64-lane mask per guard and pushes the S = 16 kernel into scratch); NR: reaction bound
// NO: 0 = bootstrap; > 0 = the guided variant for O <= NO observed dims
// CNT: the count observation term (Poisson / negative binomial, a workgroup-uniform choice inside count_term) in place of the
// Gaussian one; bootstrap only.  A compile-time argument: the Gaussian instantiations are the code they were
// RES: the residual bridge (proposal = "residual_bridge"), a form of the guided step; a compile-time argument as well
template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false, int NO = 0, bool CNT = false, bool RES = false>
__global__ void __launch_bounds__(pf_max_n(KIND, NS, NO > 0, RES)) pf_kernel(PfParams p) {
    constexpr bool GUIDED = NO > 0;
    static_assert(!(GUIDED && CNT), "the bridge proposal is derived from a Gaussian observation term");
    static_assert(GUIDED || !RES, "the residual bridge is a guided step");
    constexpr int P = KIND == 3 ? (GUIDED ? 2 * NS : 1) : KIN ? 2 * NR : NR;
    extern __shared__ __attribute__((aligned(16))) float pf_lds[];
    constexpr int S = NS, RS = S | 1;
    const int N = p.N;
    float *cum = pf_lds, *rows_s = cum + N, *red = rows_s + N * RS;
    const int j = threadIdx.x, lane = j & (kWave - 1), wave = j >> 6, nwaves = N >> 6, m = blockIdx.x;
    const uint32_t b = (uint32_t)m * (uint32_t)N + (uint32_t)j;
    const uint32_t k0 = p.key[0], k1 = p.key[1];
    float x[NS], th[P];
#pragma unroll
    for (int i = 0; i < NS; ++i) x[i] = i < S ? p.x0[(int64_t)m * S + i] : 0.f;
    if constexpr (KIND == 3 && GUIDED) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            th[i] = p.theta[(int64_t)m * p.P + i];
            th[NS + i] = softplus_f(p.theta[(int64_t)m * p.P + NS + i]) + 1e-3f;
        }
    } else if constexpr (KIND == 3) th[0] = 0.f;
    else if constexpr (KIN) crn_load_rates<NR>(th, p.theta, m, p.net.R, true);
    else em_load_theta<KIND, P>(th, p.theta, m, p.P, true);
    float loglik = 0.f;
    [[maybe_unused]] float lr = 0.f;   // guided: log (model / proposal) of the steps since the last observation
    int row_prev = 0;
    for (int k = 0; k < p.K; ++k) {
        const int row = p.rows[k];
        if (row > row_prev) {
            if constexpr (GUIDED) pf_propagate_guided<KIND, NS, NR, KIN, NO, RES>(p, x, th, row_prev, row, b, k0, k1, p.obs_values + (int64_t)k * p.O, lr);
            else pf_propagate<KIND, NS, NR, KIN, P>(p, x, th, row_prev, row, b, k0, k1, m);
            row_prev = row;
        }
        // Gaussian log-weight (the observation term of the ELBO tail kernel); NaN counts as -inf
        const float *yk = p.obs_values + (int64_t)k * p.O;
        float lw = 0.f;
        if constexpr (CNT) {
            // count log-weight: the deviance terms plus the row's constant (the terms of y alone)
            [[maybe_unused]] float unused;
            lw = p.cl.row_const[k];
            if (p.obs_matrix) {
                for (int o = 0; o < p.O; ++o) {
                    float pred = 0.f;
#pragma unroll
                    for (int i = 0; i < NS; ++i) pred += p.obs_matrix[o * S + i] * x[i];
                    lw += count_term<false>(p.cl, yk[o], pred, unused);
                }
            } else {
#pragma unroll
                for (int i = 0; i < NS; ++i) lw += count_term<false>(p.cl, yk[i], x[i], unused);
            }
        } else if (p.obs_matrix) {
            for (int o = 0; o < p.O; ++o) {
                float pred = 0.f;
#pragma unroll
                for (int i = 0; i < NS; ++i)
                    if (i < S) pred += p.obs_matrix[o * S + i] * x[i];
                const float r = yk[o] - pred;
                lw += -0.5f * r * r * p.inv_var + p.log_norm;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NS; ++i)
                if (i < S) {
                    const float r = yk[i] - x[i];
                    lw += -0.5f * r * r * p.inv_var + p.log_norm;
                }
        }
        if constexpr (GUIDED) { lw += lr; lr = 0.f; }
        if (!(lw == lw)) lw = -__builtin_inff();
        if constexpr (GUIDED)
            if (p.log_weights) p.log_weights[((int64_t)m * p.K + k) * N + j] = lw;
        if (p.particles)
#pragma unroll
            for (int i = 0; i < NS; ++i)
                if (i < S) p.particles[(((int64_t)m * p.K + k) * N + j) * S + i] = x[i];
        float mx = pf_wave_max(lw);
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = red[0];
        for (int w = 1; w < nwaves; ++w) mx = fmaxf(mx, red[w]);
        __syncthreads();
        const int64_t mk = (int64_t)m * p.K + k;
        if (mx == -__builtin_inff()) {
            // no particle has a positive weight: log p^ = -inf, the particles stay as they are
            loglik = mx;
            if (j == 0) {
                p.incr[mk] = mx; p.ess[mk] = 0.f;
                for (int i = 0; i < S; ++i) p.mean[mk * S + i] = p.std[mk * S + i] = __builtin_nanf("");
            }
            if (p.ancestors) p.ancestors[mk * N + j] = j;
            continue;
        }
        const float w = expf(lw - mx);
        // inclusive scan of w: Hillis-Steele in the wave, then a running maximum (a tree of fp32 sums is not monotone where a weight
        // is below the rounding of its neighbours' sum; the binary search and ancestors that do not decrease in j need it to be)
        float c = w;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const float t = __shfl_up(c, off, 64);
            if (lane >= off) c += t;
        }
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const float t = __shfl_up(c, off, 64);
            if (lane >= off) c = fmaxf(c, t);
        }
        if (lane == kWave - 1) red[wave] = c;
        __syncthreads();
        float base = 0.f, total = 0.f;
        for (int w2 = 0; w2 < nwaves; ++w2) {
            if (w2 == wave) base = total;
            total += red[w2];
        }
        __syncthreads();
        c += base;
        // sum w^2 and sum w x, then sum w (x - mean)^2 (two passes: no cancellation where the spread is far below the mean), four
        // dims per reduction round so that a round's operands do not crowd the state out of the registers at S = 16
        constexpr int CH = NS < 4 ? NS : 4;
        float mean[NS], s2 = 0.f;
#pragma unroll
        for (int i0 = 0; i0 < NS; i0 += CH) {
            if (i0 < S) {
                float v[CH + 1];
                v[0] = w * w;
#pragma unroll
                for (int i = 0; i < CH; ++i) v[1 + i] = (i0 + i < S && w > 0.f) ? w * x[i0 + i] : 0.f;
                pf_block_sum<CH + 1>(v, red, lane, wave, nwaves);
                s2 = v[0];
#pragma unroll
                for (int i = 0; i < CH; ++i)
                    if (i0 + i < NS) mean[i0 + i] = v[1 + i] / total;   // the last chunk of an NS that is no multiple of CH is short
            }
        }
#pragma unroll
        for (int i0 = 0; i0 < NS; i0 += CH) {
            if (i0 < S) {
                float d[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    float dx = 0.f;
                    if (i0 + i < NS) dx = x[i0 + i] - mean[i0 + i];
                    d[i] = (i0 + i < S && w > 0.f) ? w * dx * dx : 0.f;
                }
                pf_block_sum<CH>(d, red, lane, wave, nwaves);
                if (j == 0)
#pragma unroll
                    for (int i = 0; i < CH; ++i)
                        if (i0 + i < S) { p.mean[mk * S + i0 + i] = mean[i0 + i]; p.std[mk * S + i0 + i] = sqrtf(d[i] / total); }
            }
        }
        const float inc = mx + logf(total) - p.log_n;
        loglik += inc;
        if (j == 0) { p.incr[mk] = inc; p.ess[mk] = total * total / s2; }
        // systematic resampling: ancestor_j = min(#{i : C_i <= (j + u) / N C_{N-1}}, N - 1)
        cum[j] = c;
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i < S) rows_s[j * RS + i] = x[i];
        __syncthreads();
        const float u = philox_uniform(philox4x32_10(make_uint4((uint32_t)k, 0u, (uint32_t)m, 1u), k0, k1).x);
        const float tau = ((float)j + u) / (float)N * total;
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] <= tau) lo = mid + 1;
            else hi = mid;
        }
        const int anc = min(lo, N - 1);
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i < S) x[i] = rows_s[anc * RS + i];
        if (p.ancestors) p.ancestors[mk * N + j] = anc;
        __syncthreads();
    }
    if (j == 0) p.loglik[m] = loglik;
}

// the dims and the time step of a filter, checked alike for the filter and for the replay of its genealogy (guided: the bridge
// proposal's own limits first)
static inline int pf_check(bool guided, int M, int N, int S, int K, int O, double time_step) {
    VSDE_CHECK_ARG(!guided || (S >= 1 && S <= kPfGuidedMaxS), VSDE_E_BADARG, "guided particle filter: state_dim %d (1..%d supported)", S,
                   kPfGuidedMaxS);
    VSDE_CHECK_ARG(!guided || (O >= 1 && O <= kPfGuidedMaxO), VSDE_E_BADARG, "guided particle filter: obs_dim %d (1..%d supported)", O,
                   kPfGuidedMaxO);
    VSDE_CHECK_ARG(M >= 1 && K >= 1, VSDE_E_BADARG, "bad particle-filter dims M=%d K=%d", M, K);
    VSDE_CHECK_ARG(N >= kWave && N <= kPfMaxN && N % kWave == 0, VSDE_E_BADARG,
                   "particle filter: %d particles (a multiple of %d up to %d supported)", N, kWave, kPfMaxN);
    VSDE_CHECK_ARG((int64_t)M * N < ((int64_t)1 << 32), VSDE_E_BADARG, "particle filter: M N = %lld paths (below 2^32 supported)",
                   (long long)M * N);
    VSDE_CHECK_ARG(S >= 1 && S <= kPfMaxS, VSDE_E_BADARG, "particle filter: state_dim %d (1..%d supported)", S, kPfMaxS);
    VSDE_CHECK_ARG(O >= 1 && O <= kPfMaxO, VSDE_E_BADARG, "particle filter: obs_dim %d (1..%d supported)", O, kPfMaxO);
    VSDE_CHECK_ARG(time_step > 0, VSDE_E_BADARG, "bad variance / time_step");
    return 0;
}

template <class Kern> static int pf_launch(Kern kern, const PfParams &p, void *stream, int max_n) {
    VSDE_CHECK_ARG(p.N <= max_n, VSDE_E_BADARG, "particle filter: %d particles (up to %d supported at state_dim %d of this SDE)", p.N,
                   max_n, p.S);
    const size_t lds = ((size_t)p.N * ((p.S | 1) + 1) + kPfRed) * sizeof(float);
    if (lds > 64 * 1024)
        VSDE_CHECK_HIP(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kern, dim3(p.M), dim3(p.N), lds, (hipStream_t)stream, p);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

// One body for the vsde_*particle_filter entry points: any route, bootstrap or guided (the bridge proposal; log_weights is its
// optional output), Gaussian or (ca, bootstrap only) count observation term.  Every check comes before the first HIP call.
// RES: the residual form of the guided filter (guided must be set); a translation unit instantiates the kernels of one RES only
template <bool RES = false>
static int particle_filter(const SdeRoute &rt, bool guided, const CountArgs *ca, int M, int N, int S, int P, int K, int O,
                           const float *x0, const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                           double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                           float *log_likelihood, float *increments, float *ess, float *filtered_mean, float *filtered_std,
                           float *particles, int *ancestors, float *log_weights, void *stream) {
    PfParams p = {};
    int rc = route_check(rt, S, P, p.net);
    if (!rc) rc = pf_check(guided, M, N, S, K, O, time_step);
    if (!rc) rc = pf_obs(p, S, O, obs_values, obs_matrix, variance);
    if (rc) return rc;
    VSDE_CHECK_ARG(x0 && theta && obs_rows && obs_values && key && log_likelihood && increments && ess && filtered_mean && filtered_std,
                   VSDE_E_BADARG, "NULL argument");
    if ((rc = count_fill(p.cl, ca, K))) return rc;
    pf_fill(p, M, N, S, P, K, O, x0, theta, obs_rows, key, time_step, positive_mask_host);
    p.loglik = log_likelihood; p.incr = increments; p.ess = ess; p.mean = filtered_mean; p.std = filtered_std;
    p.particles = particles; p.ancestors = ancestors; p.log_weights = log_weights; p.log_n = (float)log((double)N);
    // the instantiation of (KIND, NS, NR, KIN) for the call: guided at the bound NO = 2 or 4 of its observation dim (S <= 4), or
    // bootstrap with either observation term
    if constexpr (RES) {
        return route_dispatch<kPfGuidedMaxS, kPfGuidedMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
            constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value, max_n = pf_max_n(KIND, NS, true, true);
            constexpr bool KIN = decltype(kin)::value;
            if (O <= 2) return pf_launch(pf_kernel<KIND, NS, NR, KIN, 2, false, true>, p, stream, max_n);
            return pf_launch(pf_kernel<KIND, NS, NR, KIN, 4, false, true>, p, stream, max_n);
        });
    } else {
        if (guided)
            return route_dispatch<kPfGuidedMaxS, kPfGuidedMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
                constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value, max_n = pf_max_n(KIND, NS, true);
                constexpr bool KIN = decltype(kin)::value;
                if (O <= 2) return pf_launch(pf_kernel<KIND, NS, NR, KIN, 2>, p, stream, max_n);
                return pf_launch(pf_kernel<KIND, NS, NR, KIN, 4>, p, stream, max_n);
            });
        return route_dispatch<kPfMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
            constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value, max_n = pf_max_n(KIND, NS);
            constexpr bool KIN = decltype(kin)::value;
            if (ca) return pf_launch(pf_kernel<KIND, NS, NR, KIN, 0, true>, p, stream, max_n);
            return pf_launch(pf_kernel<KIND, NS, NR, KIN, 0, false>, p, stream, max_n);
        });
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Replay of the filter's genealogy (viforsdes_amd/inference/particle_smoother.py is the specification): D posterior paths per filter
// from the stored particles and ancestors.  A thread per (observation k, filter m, draw d), k slowest, so the lanes of a wave run
// segments of the same length: it walks its draw's lineage from the last observation down to k through `ancestors` (at most K
// loads), starts from the stored particle its lineage had at observation k - 1 (x0 for k = 0) and repeats the grid steps
// obs_rows[k-1] .. obs_rows[k] - 1 with the noise of its slot at k: pf_propagate / pf_propagate_guided with a store hook, so step,
// clamp and Philox block structure are the filter's own.  A thread is not tied to a particle: 256-thread workgroups (512 VGPRs a
// lane) keep every instantiation out of scratch.
struct RpParams {
    int D, T;
    const float *particles;
    const int *ancestors, *last_slot;
    float *paths;
    int *lineage;
};

template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false, int NO = 0, bool RES = false>
__global__ void __launch_bounds__(kRpThreads) rp_kernel(PfParams p, RpParams r) {
    constexpr bool GUIDED = NO > 0;
    constexpr int P = KIND == 3 ? (GUIDED ? 2 * NS : 1) : KIN ? 2 * NR : NR;
    constexpr int S = NS;
    const int64_t md = (int64_t)p.M * r.D, g = (int64_t)blockIdx.x * kRpThreads + threadIdx.x;
    if (g >= md * p.K) return;
    const int k = (int)(g / md), N = p.N;
    const int64_t q = g - (int64_t)k * md;   // m D + d
    const int m = (int)(q / r.D);
    const int t0 = k ? p.rows[k - 1] : 0, t1 = p.rows[k];
    if (t0 < 0 || t1 < t0 || t1 > r.T) return;   // rows that decrease or pass the paths' T: nothing is written
    float *path = r.paths + q * ((int64_t)r.T + 1) * S;
    int slot = r.last_slot[q];
    if (slot < 0 || slot >= N) {
        // a dead filter has no smoothing sample
        for (int t = k ? t0 + 1 : 0; t <= t1; ++t)
#pragma unroll
            for (int i = 0; i < NS; ++i) path[(int64_t)t * S + i] = __builtin_nanf("");
        if (r.lineage) r.lineage[q * p.K + k] = -1;
        return;
    }
    // ancestors are slots of the same filter; the clamp keeps a corrupt entry inside its row
    const int *anc = r.ancestors + (int64_t)m * p.K * N;
    for (int kk = p.K - 1; kk > k; --kk) slot = min(max(anc[(int64_t)(kk - 1) * N + slot], 0), N - 1);
    if (r.lineage) r.lineage[q * p.K + k] = slot;
    float x[NS], th[P];
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) path[i] = x[i] = p.x0[(int64_t)m * S + i];
    } else {
        const int prev = min(max(anc[(int64_t)(k - 1) * N + slot], 0), N - 1);
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = r.particles[(((int64_t)m * p.K + k - 1) * N + prev) * S + i];
    }
    if (t1 == t0) return;
    if constexpr (KIND == 3 && GUIDED) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            th[i] = p.theta[(int64_t)m * p.P + i];
            th[NS + i] = softplus_f(p.theta[(int64_t)m * p.P + NS + i]) + 1e-3f;
        }
    } else if constexpr (KIND == 3) th[0] = 0.f;
    else if constexpr (KIN) crn_load_rates<NR>(th, p.theta, m, p.net.R, true);
    else em_load_theta<KIND, P>(th, p.theta, m, p.P, true);
    const uint32_t b = (uint32_t)m * (uint32_t)N + (uint32_t)slot, k0 = p.key[0], k1 = p.key[1];
    const RpStore st{path, S};
    if constexpr (GUIDED) {
        float lr = 0.f;
        pf_propagate_guided<KIND, NS, NR, KIN, NO, RES>(p, x, th, t0, t1, b, k0, k1, p.obs_values + (int64_t)k * p.O, lr, st);
    } else {
        pf_propagate<KIND, NS, NR, KIN, P>(p, x, th, t0, t1, b, k0, k1, m, st);
    }
}

// One body for the vsde_*filter_replay entry points: any route, plain or guided (the bridge proposal reads the observation model
// again; the plain forwarders pass none).  Every check comes before the first HIP call.  RES: as in particle_filter
template <bool RES = false>
static int filter_replay(const SdeRoute &rt, bool guided, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0,
                         const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                         const uint32_t *key, double time_step, const uint8_t *positive_mask_host, const float *particles,
                         const int *ancestors, const int *last_slot, float *paths, int *lineage, void *stream) {
    PfParams p = {};
    int rc = route_check(rt, S, P, p.net);
    if (!rc) rc = pf_check(guided, M, N, S, K, O, time_step);
    if (!rc && guided) rc = pf_obs(p, S, O, obs_values, obs_matrix, variance);
    if (rc) return rc;
    VSDE_CHECK_ARG(D >= 1, VSDE_E_BADARG, "filter replay: %d draws per filter (>= 1 supported)", D);
    VSDE_CHECK_ARG(T >= 0, VSDE_E_BADARG, "filter replay: %d grid steps", T);
    VSDE_CHECK_ARG((int64_t)M * D * K < ((int64_t)1 << 31), VSDE_E_BADARG, "filter replay: M D K = %lld segments (below 2^31 supported)",
                   (long long)M * D * K);
    VSDE_CHECK_ARG(x0 && theta && obs_rows && key && particles && ancestors && last_slot && paths && (obs_values || !guided),
                   VSDE_E_BADARG, "NULL argument");
    pf_fill(p, M, N, S, P, K, O, x0, theta, obs_rows, key, time_step, positive_mask_host);
    const RpParams r = {D, T, particles, ancestors, last_slot, paths, lineage};
    const auto launch = [&](auto kern) {
        const int64_t threads = (int64_t)M * D * K;
        hipLaunchKernelGGL(kern, dim3((unsigned)((threads + kRpThreads - 1) / kRpThreads)), dim3(kRpThreads), 0, (hipStream_t)stream, p, r);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    };
    if constexpr (RES) {
        return route_dispatch<kPfGuidedMaxS, kPfGuidedMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
            constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value;
            if (O <= 2) return launch(rp_kernel<KIND, NS, NR, decltype(kin)::value, 2, true>);
            return launch(rp_kernel<KIND, NS, NR, decltype(kin)::value, 4, true>);
        });
    } else {
        if (guided)
            return route_dispatch<kPfGuidedMaxS, kPfGuidedMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
                constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value;
                if (O <= 2) return launch(rp_kernel<KIND, NS, NR, decltype(kin)::value, 2>);
                return launch(rp_kernel<KIND, NS, NR, decltype(kin)::value, 4>);
            });
        return route_dispatch<kPfMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
            return launch(rp_kernel<decltype(kind)::value, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>);
        });
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Replay of B carried path records (viforsdes_amd/inference/particle_mcmc.py is the specification): what a PMMH chain keeps of the
// one trajectory it accepted with its theta.  A record is self-contained: its start state, theta and filter key, the state its
// lineage had at every observation (anchors) and the noise path of every segment, so nothing of a filter's store is read.  A
// thread per (observation k, record b), k slowest as in rp_kernel; the step is the same pf_propagate / pf_propagate_guided call.
struct ArParams {
    int B, T;
    const float *anchors;          // [B][K][S]
    const uint32_t *noise_path;    // [B][K]
    const uint32_t *keys;          // [B][2]
    float *paths;                  // [B][T + 1][S]
};

constexpr uint32_t kArDeadPath = 0xFFFFFFFFu;

template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false, int NO = 0, bool RES = false>
__global__ void __launch_bounds__(kRpThreads) ar_kernel(PfParams p, ArParams r) {
    constexpr bool GUIDED = NO > 0;
    constexpr int P = KIND == 3 ? (GUIDED ? 2 * NS : 1) : KIN ? 2 * NR : NR;
    constexpr int S = NS;
    const int64_t g = (int64_t)blockIdx.x * kRpThreads + threadIdx.x;
    if (g >= (int64_t)r.B * p.K) return;
    const int k = (int)(g / r.B), b = (int)(g - (int64_t)k * r.B);
    const int t0 = k ? p.rows[k - 1] : 0, t1 = p.rows[k];
    if (t0 < 0 || t1 < t0 || t1 > r.T) return;   // rows that decrease or pass the paths' T: nothing is written
    float *path = r.paths + (int64_t)b * ((int64_t)r.T + 1) * S;
    const uint32_t *noise = r.noise_path + (int64_t)b * p.K;
    if (noise[p.K - 1] == kArDeadPath) {
        // a dead record has no path
        for (int t = k ? t0 + 1 : 0; t <= t1; ++t)
#pragma unroll
            for (int i = 0; i < NS; ++i) path[(int64_t)t * S + i] = __builtin_nanf("");
        return;
    }
    float x[NS], th[P];
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < NS; ++i) path[i] = x[i] = p.x0[(int64_t)b * S + i];
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) x[i] = r.anchors[((int64_t)b * p.K + k - 1) * S + i];
    }
    if (t1 == t0) return;
    if constexpr (KIND == 3 && GUIDED) {
#pragma unroll
        for (int i = 0; i < NS; ++i) {
            th[i] = p.theta[(int64_t)b * p.P + i];
            th[NS + i] = softplus_f(p.theta[(int64_t)b * p.P + NS + i]) + 1e-3f;
        }
    } else if constexpr (KIND == 3) th[0] = 0.f;
    else if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, p.net.R, true);
    else em_load_theta<KIND, P>(th, p.theta, b, p.P, true);
    const uint32_t nb = noise[k], k0 = r.keys[2 * (int64_t)b], k1 = r.keys[2 * (int64_t)b + 1];
    const RpStore st{path, S};
    if constexpr (GUIDED) {
        float lr = 0.f;
        pf_propagate_guided<KIND, NS, NR, KIN, NO, RES>(p, x, th, t0, t1, nb, k0, k1, p.obs_values + (int64_t)k * p.O, lr, st);
    } else {
        pf_propagate<KIND, NS, NR, KIN, P>(p, x, th, t0, t1, nb, k0, k1, b, st);
    }
}

// One body for the vsde_*anchored_replay entry points: any route, plain or guided.  Every check comes before the first HIP call.
// RES: as in particle_filter
template <bool RES = false>
static int anchored_replay(const SdeRoute &rt, bool guided, int B, int S, int P, int K, int O, int T, const float *x0,
                           const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                           const float *anchors, const uint32_t *noise_path, const uint32_t *keys, double time_step,
                           const uint8_t *positive_mask_host, float *paths, void *stream) {
    PfParams p = {};
    int rc = route_check(rt, S, P, p.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(!guided || (S >= 1 && S <= kPfGuidedMaxS), VSDE_E_BADARG, "guided anchored replay: state_dim %d (1..%d supported)", S,
                   kPfGuidedMaxS);
    VSDE_CHECK_ARG(!guided || (O >= 1 && O <= kPfGuidedMaxO), VSDE_E_BADARG, "guided anchored replay: obs_dim %d (1..%d supported)", O,
                   kPfGuidedMaxO);
    VSDE_CHECK_ARG(B >= 1 && K >= 1, VSDE_E_BADARG, "anchored replay: bad dims B=%d K=%d", B, K);
    VSDE_CHECK_ARG(S >= 1 && S <= kPfMaxS, VSDE_E_BADARG, "anchored replay: state_dim %d (1..%d supported)", S, kPfMaxS);
    VSDE_CHECK_ARG(O >= 1 && O <= kPfMaxO, VSDE_E_BADARG, "anchored replay: obs_dim %d (1..%d supported)", O, kPfMaxO);
    VSDE_CHECK_ARG(time_step > 0, VSDE_E_BADARG, "bad variance / time_step");
    if (guided && (rc = pf_obs(p, S, O, obs_values, obs_matrix, variance))) return rc;
    VSDE_CHECK_ARG(T >= 0, VSDE_E_BADARG, "anchored replay: %d grid steps", T);
    VSDE_CHECK_ARG((int64_t)B * K < ((int64_t)1 << 31), VSDE_E_BADARG, "anchored replay: B K = %lld segments (below 2^31 supported)",
                   (long long)B * K);
    VSDE_CHECK_ARG(x0 && theta && obs_rows && anchors && noise_path && keys && paths && (obs_values || !guided), VSDE_E_BADARG,
                   "NULL argument");
    pf_fill(p, B, 0, S, P, K, O, x0, theta, obs_rows, nullptr, time_step, positive_mask_host);
    const ArParams r = {B, T, anchors, noise_path, keys, paths};
    const auto launch = [&](auto kern) {
        const int64_t threads = (int64_t)B * K;
        hipLaunchKernelGGL(kern, dim3((unsigned)((threads + kRpThreads - 1) / kRpThreads)), dim3(kRpThreads), 0, (hipStream_t)stream, p, r);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    };
    if constexpr (RES) {
        return route_dispatch<kPfGuidedMaxS, kPfGuidedMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
            constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value;
            if (O <= 2) return launch(ar_kernel<KIND, NS, NR, decltype(kin)::value, 2, true>);
            return launch(ar_kernel<KIND, NS, NR, decltype(kin)::value, 4, true>);
        });
    } else {
        if (guided)
            return route_dispatch<kPfGuidedMaxS, kPfGuidedMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
                constexpr int KIND = decltype(kind)::value, NS = decltype(ns)::value, NR = decltype(nr)::value;
                if (O <= 2) return launch(ar_kernel<KIND, NS, NR, decltype(kin)::value, 2>);
                return launch(ar_kernel<KIND, NS, NR, decltype(kin)::value, 4>);
            });
        return route_dispatch<kPfMaxS>(rt, S, p.net.R, [&](auto kind, auto ns, auto nr, auto kin) {
            return launch(ar_kernel<decltype(kind)::value, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>);
        });
    }
}

}  // namespace vsde
