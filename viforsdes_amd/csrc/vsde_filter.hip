// Bootstrap particle filter of the built-in SDEs (gfx950): log p^(y | theta) of the Euler-Maruyama-discretised model with a
// Gaussian or (template argument CNT) a Poisson / negative-binomial observation term, for M parameter vectors at once (viforsdes_amd/inference/particle_filter.py is the specification).
// One launch runs whole filters: a workgroup per theta, a thread per particle; the particle's state, theta and the running
// log-likelihood stay in registers from the first Euler step to the last.  Neither noise nor trajectory is stored: the normals come
// from the forecast kernel's Philox stream (vsde_sde_step.h: fc_normals) with path index b = m N + j.
// At an observation: the log-weight in registers; max, sum w^2 and sum w x by wave butterflies and one LDS stage; an inclusive
// scan of the weights (wave scan by cross-lane moves, wave totals through LDS); cumulative sums and particle states go to LDS
// (row stride S | 1: the gather below is not a bank conflict), every thread finds its ancestor by binary search over the cumulative
// sums (systematic resampling, one uniform per (filter, observation)) and reads that state row.
// The guided variant (template argument NO > 0: proposal = "bridge", S <= 4, O <= NO in {2, 4}) replaces the Euler step by the
// modified-diffusion-bridge step of the specification (pf_bridge_step) and carries the log-ratio model / proposal in one more
// register to the observation; everything from the log-weight on is the same code.
// LDS (dynamic): N cumulative sums + N (S | 1) state floats + 16 x 18 reduction slots: 73 KiB at N = 1024, S = 16.
// The particle smoother's replay kernel (rp_kernel, at the end of the namespace) runs single segments of a filter again from the
// stored particles and ancestors, through the same pf_propagate / pf_propagate_guided with a store hook.  That step code and the
// argument block live in vsde_filter_step.h: the replay of carried path records (particle MCMC with paths: vsde_anchored.hip)
// shares them from a translation unit of its own.
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
template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false, int NO = 0, bool CNT = false>
__global__ void __launch_bounds__(pf_max_n(KIND, NS, NO > 0)) pf_kernel(PfParams p) {
    constexpr bool GUIDED = NO > 0;
    static_assert(!(GUIDED && CNT), "the bridge proposal is derived from a Gaussian observation term");
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
            if constexpr (GUIDED) pf_propagate_guided<KIND, NS, NR, KIN, NO>(p, x, th, row_prev, row, b, k0, k1, p.obs_values + (int64_t)k * p.O, lr);
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
                for (int i = 0; i < CH; ++i) mean[i0 + i] = v[1 + i] / total;
            }
        }
#pragma unroll
        for (int i0 = 0; i0 < NS; i0 += CH) {
            if (i0 < S) {
                float d[CH];
#pragma unroll
                for (int i = 0; i < CH; ++i) {
                    const float dx = x[i0 + i] - mean[i0 + i];
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
static int pf_check(bool guided, int M, int N, int S, int K, int O, double time_step) {
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

template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false, int NO = 0>
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
        pf_propagate_guided<KIND, NS, NR, KIN, NO>(p, x, th, t0, t1, b, k0, k1, p.obs_values + (int64_t)k * p.O, lr, st);
    } else {
        pf_propagate<KIND, NS, NR, KIN, P>(p, x, th, t0, t1, b, k0, k1, m, st);
    }
}

// One body for the vsde_*filter_replay entry points: any route, plain or guided (the bridge proposal reads the observation model
// again; the plain forwarders pass none).  Every check comes before the first HIP call.
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

}  // namespace vsde

using namespace vsde;

// The exported functions: each builds its route and forwards to the one body of its operation
extern "C" int vsde_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                                    const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                    const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                    float *log_likelihood, float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                    float *particles, int *ancestors, void *stream) {
    return particle_filter(SdeRoute{kind}, false, nullptr, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, variance,
                           key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                           particles, ancestors, nullptr, stream);
}

extern "C" int vsde_crn_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                        const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                        double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                        float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                        float *filtered_std, float *particles, int *ancestors, void *stream) {
    return particle_filter(crn_route(net), false, nullptr, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, variance,
                           key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                           particles, ancestors, nullptr, stream);
}

extern "C" int vsde_crn_kinetic_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                                int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                                const float *obs_values, const float *obs_matrix, double variance,
                                                const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                                float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                                float *filtered_std, float *particles, int *ancestors, void *stream) {
    return particle_filter(crn_route(net, kin), false, nullptr, M, N, S, P, K, O, x0, rates, obs_rows, obs_values, obs_matrix,
                           variance, key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                           particles, ancestors, nullptr, stream);
}

extern "C" int vsde_guided_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                                           const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                           const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                           float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                           float *filtered_std, float *particles, int *ancestors, float *log_weights, void *stream) {
    return particle_filter(SdeRoute{kind}, true, nullptr, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, variance,
                           key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                           particles, ancestors, log_weights, stream);
}

extern "C" int vsde_crn_guided_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                               const float *theta, const int *obs_rows, const float *obs_values,
                                               const float *obs_matrix, double variance, const uint32_t *key, double time_step,
                                               const uint8_t *positive_mask_host, float *log_likelihood, float *increments,
                                               float *ess, float *filtered_mean, float *filtered_std, float *particles,
                                               int *ancestors, float *log_weights, void *stream) {
    return particle_filter(crn_route(net), true, nullptr, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, variance,
                           key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                           particles, ancestors, log_weights, stream);
}

extern "C" int vsde_crn_kinetic_guided_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                       int P, int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                                       const float *obs_values, const float *obs_matrix, double variance,
                                                       const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                                       float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                                       float *filtered_std, float *particles, int *ancestors, float *log_weights,
                                                       void *stream) {
    return particle_filter(crn_route(net, kin), true, nullptr, M, N, S, P, K, O, x0, rates, obs_rows, obs_values, obs_matrix,
                           variance, key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                           particles, ancestors, log_weights, stream);
}

// The bootstrap filter with a count observation term: the CNT instantiations
extern "C" int vsde_count_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                                          const int *obs_rows, const float *obs_values, const float *obs_matrix, int lik_kind,
                                          double scale, double dispersion, const float *row_const, const uint32_t *key,
                                          double time_step, const uint8_t *positive_mask_host, float *log_likelihood,
                                          float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                          float *particles, int *ancestors, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return particle_filter(SdeRoute{kind}, false, &ca, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, 1.0, key,
                           time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std, particles,
                           ancestors, nullptr, stream);
}

extern "C" int vsde_crn_count_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                              const float *theta, const int *obs_rows, const float *obs_values,
                                              const float *obs_matrix, int lik_kind, double scale, double dispersion,
                                              const float *row_const, const uint32_t *key, double time_step,
                                              const uint8_t *positive_mask_host, float *log_likelihood, float *increments,
                                              float *ess, float *filtered_mean, float *filtered_std, float *particles,
                                              int *ancestors, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return particle_filter(crn_route(net), false, &ca, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, 1.0, key,
                           time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std, particles,
                           ancestors, nullptr, stream);
}

extern "C" int vsde_crn_kinetic_count_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                      int P, int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                                      const float *obs_values, const float *obs_matrix, int lik_kind, double scale,
                                                      double dispersion, const float *row_const, const uint32_t *key,
                                                      double time_step, const uint8_t *positive_mask_host, float *log_likelihood,
                                                      float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                                      float *particles, int *ancestors, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return particle_filter(crn_route(net, kin), false, &ca, M, N, S, P, K, O, x0, rates, obs_rows, obs_values, obs_matrix, 1.0, key,
                           time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std, particles,
                           ancestors, nullptr, stream);
}

// Replay of the filter's genealogy: posterior paths from the particles and ancestors the entry points above stored
extern "C" int vsde_filter_replay(int kind, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0, const float *theta,
                                  const int *obs_rows, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                  const float *particles, const int *ancestors, const int *last_slot, float *paths, int *lineage,
                                  void *stream) {
    return filter_replay(SdeRoute{kind}, false, M, N, S, P, K, O, D, T, x0, theta, obs_rows, nullptr, nullptr, 1.0, key, time_step,
                         positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_crn_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, int D, int T,
                                      const float *x0, const float *theta, const int *obs_rows, const uint32_t *key, double time_step,
                                      const uint8_t *positive_mask_host, const float *particles, const int *ancestors,
                                      const int *last_slot, float *paths, int *lineage, void *stream) {
    return filter_replay(crn_route(net), false, M, N, S, P, K, O, D, T, x0, theta, obs_rows, nullptr, nullptr, 1.0, key, time_step,
                         positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_crn_kinetic_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                              int K, int O, int D, int T, const float *x0, const float *rates, const int *obs_rows,
                                              const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                              const float *particles, const int *ancestors, const int *last_slot, float *paths,
                                              int *lineage, void *stream) {
    return filter_replay(crn_route(net, kin), false, M, N, S, P, K, O, D, T, x0, rates, obs_rows, nullptr, nullptr, 1.0, key,
                         time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_guided_filter_replay(int kind, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0,
                                         const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                         double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                         const float *particles, const int *ancestors, const int *last_slot, float *paths,
                                         int *lineage, void *stream) {
    return filter_replay(SdeRoute{kind}, true, M, N, S, P, K, O, D, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, key,
                         time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_crn_guided_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, int D, int T,
                                             const float *x0, const float *theta, const int *obs_rows, const float *obs_values,
                                             const float *obs_matrix, double variance, const uint32_t *key, double time_step,
                                             const uint8_t *positive_mask_host, const float *particles, const int *ancestors,
                                             const int *last_slot, float *paths, int *lineage, void *stream) {
    return filter_replay(crn_route(net), true, M, N, S, P, K, O, D, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, key,
                         time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_crn_kinetic_guided_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                     int P, int K, int O, int D, int T, const float *x0, const float *rates,
                                                     const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                                     double variance, const uint32_t *key, double time_step,
                                                     const uint8_t *positive_mask_host, const float *particles, const int *ancestors,
                                                     const int *last_slot, float *paths, int *lineage, void *stream) {
    return filter_replay(crn_route(net, kin), true, M, N, S, P, K, O, D, T, x0, rates, obs_rows, obs_values, obs_matrix, variance,
                         key, time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}
