// Bootstrap particle filter on the exact jump process of a reaction network (gfx950): log p^(y | theta) with particles that are
// Gillespie trajectories on integer copy numbers, for M parameter vectors at once.  No time step, no diffusion approximation.
// viforsdes_amd/inference/jump_filter.py is the specification.
//
// One launch runs whole filters: a workgroup per theta, a thread per particle (N a multiple of 64).  The int32 state x [S], the
// constants, the cumulative propensities, the float64 clock and the running log-likelihood live in registers from the first event
// to the last.
//
// Segment k (T_{k-1}, T_k] of particle slot j of filter m, path b = m N + j: the clock restarts at exactly T_{k-1} (T_{-1} = 0; the
// waiting times are memoryless) and the event counter at 0.  Event e is jump_kernel's (vsde_jump.hip): a_j = crn_jump_propensity,
// c_j = a_0 + .. + a_j in fp32, a NaN / infinite / negative a_j or an infinite a0 -> stopped (status 2); tau = -logf(u1) / a0,
// the segment ends as soon as T_k < t + (double)tau (a0 == 0: at once, the state is absorbed); else the reaction is the smallest
// j with u2 a0 < c_j (none: the last j with a_j > 0), x += nu_j.  (u1, u2) = uniforms 2 (e & 1), 2 (e & 1) + 1 of
// philox4x32_10({e >> 1, k, b, 7}, key): the jump process's stream with the segment in the second counter word.  The only event
// loop counts e up to max_events: a particle that has fired max_events events short of T_k stops (status 1).  A stopped particle
// keeps its state, weighs -inf at observation k, and carries on from that state at T_k only if the whole filter is dead.
// The lanes of a wave wait for their slowest particle at every observation.
//
// Observation k follows pf_kernel's order of operations (vsde_filter_kernels.h) on (float)x: the log-weight (Gaussian, Poisson or
// negative binomial: a workgroup-uniform run-time choice, the event loop dominates), wave max, Hillis-Steele scan plus running
// maximum, wave totals through LDS, two-pass moments four dims per round, binary search over the cumulative sums.  The LDS rows
// that resampling gathers hold the int32 bits of the state, not a float conversion: 2^30 + 1 does not survive fp32.
// LDS (dynamic): N cumulative sums + N (S | 1) state words + 16 x 18 reduction slots: 41 KiB at N = 1024, S = 8.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vsde_filter_kernels.h"

namespace vsde {

constexpr int kJfMaxEvents = 1 << 23;   // vsde_jump.hip: kJumpMaxEvents (x0 <= 2^30 and |nu| <= 127: the int32 state cannot overflow)

// Particles per filter an instantiation is built for (_hip.jump_filter_max_particles restates it).  A 1024-thread workgroup leaves
// 128 VGPRs a lane, and every instantiation fits: the widest (S = 8, the rate-law form at 16 reactions: 32 constants and 16
// cumulative sums next to the state) takes 108, none has scratch.  The arguments are what a cap would depend on.
constexpr int jf_max_n(int S, int NR, bool kin) { return kPfMaxN; }

struct JfParams {
    int M, N, S, P, K, O, max_events, lik;   // lik: VSDE_LIK_GAUSSIAN / POISSON / NEGATIVE_BINOMIAL
    const int32_t *x0;         // [M][S]
    const float *theta;        // [M][P]: k (P = R), or the effective constants (k, K) (P = 2R)
    const double *times;       // [K] non-decreasing observation times
    const float *obs_values;   // [K][O]
    const float *obs_matrix;   // [O][S] or NULL (O == S)
    const uint32_t *key;       // 2 words
    float *loglik, *incr, *ess, *mean, *std, *mean_events;
    int32_t *stopped;
    int32_t *particles;        // [M][K][N][S] or NULL
    int *ancestors;            // [M][K][N] or NULL
    float *log_weights;        // [M][K][N] or NULL
    int32_t *events;           // [M][K][N] or NULL
    float inv_var, log_norm, log_n;
    CountLik cl;
    uint32_t orders[kCrnMaxR];   // reactant row of reaction j, 2 bits per species (crn_pack_orders)
    uint32_t nu[kCrnMaxR][2];    // net change of reaction j, one int8 per species: species 0..3, 4..7
    CrnNet net;
};

// The kernel's argument block through a pointer the compiler cannot see through: loads from it stay where they are written (K times
// a launch, at the observations) instead of being hoisted above the event loop, where some 60 loop-invariant SGPRs of pointers and
// masks would be spilled to VGPR lanes around every segment.  The block is the kernel's only argument: offset 0 of the segment
__device__ __forceinline__ const JfParams &jf_args_again() {
    uint64_t a = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return *(const JfParams *)(const __attribute__((address_space(4))) void *)a;
}

template <int S, int NR, bool KIN> __global__ void __launch_bounds__(jf_max_n(S, NR, KIN)) jf_kernel(JfParams p) {
    constexpr int P = KIN ? 2 * NR : NR, RS = S | 1;
    extern __shared__ __attribute__((aligned(16))) float jf_lds[];
    const int N = p.N, R = p.net.R;
    float *cum = jf_lds, *red = cum + N + N * RS;
    int *rows_s = reinterpret_cast<int *>(cum + N);
    const int j = threadIdx.x, lane = j & (kWave - 1), wave = j >> 6, nwaves = N >> 6, m = blockIdx.x;
    const uint32_t b = (uint32_t)m * (uint32_t)N + (uint32_t)j;
    const uint32_t k0 = p.key[0], k1 = p.key[1];
    int x[S];
    float th[P];
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = p.x0[(int64_t)m * S + i];
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, m, R, true);
    else em_load_theta<4, P>(th, p.theta, m, p.P, true);
    float loglik = 0.f;
    double t_prev = 0.0;
#pragma unroll 1
    for (int k = 0; k < p.K; ++k) {
        // ---- the segment (t_prev, t_k]: jump_kernel's event, one output time
        const double t_k = p.times[k];
        double t = t_prev;
        int ne = 0, st = 1;                // st: the status if the loop runs out of events
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
        for (int e = 0; e < p.max_events; ++e) {
            float xf[S], c[NR];
#pragma unroll
            for (int i = 0; i < S; ++i) xf[i] = (float)x[i];
            float acc = 0.f;
            bool bad = false;
            int jlast = 0;                     // the last reaction with a_j > 0
#pragma unroll
            for (int jj = 0; jj < NR; ++jj) {
                if (jj < R) {
                    const float a = crn_jump_propensity<S, NR, KIN>(p.net, p.orders[jj], jj, x, xf, th);
                    bad = bad || !(a >= 0.f) || a == INFINITY;
                    if (a > 0.f) jlast = jj;
                    acc += a;
                }
                c[jj] = acc;
            }
            const float a0 = acc;
            if (bad || a0 == INFINITY) { st = 2; break; }
            if ((e & 1) == 0) w = philox4x32_10(make_uint4((uint32_t)e >> 1, (uint32_t)k, b, 7u), k0, k1);
            const float u1 = philox_uniform((e & 1) ? w.z : w.x), u2 = philox_uniform((e & 1) ? w.w : w.y);
            const double tn = a0 == 0.f ? (double)INFINITY : t + (double)(-logf(u1) / a0);
            if (t_k < tn) { st = 0; break; }
            const float thr = u2 * a0;
            int js = -1;
#pragma unroll
            for (int jj = NR - 1; jj >= 0; --jj)
                if (jj < R && thr < c[jj]) js = jj;
            if (js < 0) js = jlast;
            // the chosen row (8 int8 in two words) by compare-selects over the uniform table: indexing the table by the lane's js
            // would go to scratch
            uint32_t lo = 0u, hi = 0u;
#pragma unroll
            for (int jj = 0; jj < NR; ++jj)
                if (jj == js) {
                    lo = p.nu[jj][0];
                    if constexpr (S > 4) hi = p.nu[jj][1];
                }
#pragma unroll
            for (int i = 0; i < S; ++i) x[i] += (int)(int8_t)((i < 4 ? lo : hi) >> (8 * (i & 3)));
            t = tn;
            ++ne;
        }
        t_prev = t_k;
        // ---- observation k: pf_kernel's stage on (float)x; a stopped particle weighs -inf.  Its arguments are read again here
        // (jf_args_again): hoisted out of both loops they would crowd the event loop's tables out of the SGPRs
        const JfParams &q = jf_args_again();
        float xf[S];
#pragma unroll
        for (int i = 0; i < S; ++i) xf[i] = (float)x[i];
        const float *yk = q.obs_values + (int64_t)k * q.O;
        float lw = 0.f;
        if (q.lik != VSDE_LIK_GAUSSIAN) {
            // count log-weight: the deviance terms plus the row's constant (the terms of y alone)
            [[maybe_unused]] float unused;
            lw = q.cl.row_const[k];
            if (q.obs_matrix) {
#pragma unroll 1
                for (int o = 0; o < q.O; ++o) {
                    float pred = 0.f;
#pragma unroll
                    for (int i = 0; i < S; ++i) pred += q.obs_matrix[o * S + i] * xf[i];
                    lw += count_term<false>(q.cl, yk[o], pred, unused);
                }
            } else {
#pragma unroll
                for (int i = 0; i < S; ++i) lw += count_term<false>(q.cl, yk[i], xf[i], unused);
            }
        } else if (q.obs_matrix) {
#pragma unroll 1
            for (int o = 0; o < q.O; ++o) {
                float pred = 0.f;
#pragma unroll
                for (int i = 0; i < S; ++i) pred += q.obs_matrix[o * S + i] * xf[i];
                const float r = yk[o] - pred;
                lw += -0.5f * r * r * q.inv_var + q.log_norm;
            }
        } else {
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const float r = yk[i] - xf[i];
                lw += -0.5f * r * r * q.inv_var + q.log_norm;
            }
        }
        if (!(lw == lw) || st != 0) lw = -__builtin_inff();
        const int64_t mk = (int64_t)m * q.K + k;
        if (q.log_weights) q.log_weights[mk * N + j] = lw;
        if (q.events) q.events[mk * N + j] = ne;
        if (q.particles)
#pragma unroll
            for (int i = 0; i < S; ++i) q.particles[(mk * N + j) * S + i] = x[i];
        {
            // the segment's record: stopped particles (exact in fp32: at most 1024) and events per particle
            float v[2] = {st != 0 ? 1.f : 0.f, (float)ne};
            pf_block_sum<2>(v, red, lane, wave, nwaves);
            if (j == 0) { q.stopped[mk] = (int32_t)v[0]; q.mean_events[mk] = v[1] / (float)N; }
        }
        float mx = pf_wave_max(lw);
        if (lane == 0) red[wave] = mx;
        __syncthreads();
        mx = red[0];
        for (int w2 = 1; w2 < nwaves; ++w2) mx = fmaxf(mx, red[w2]);
        __syncthreads();
        if (mx == -__builtin_inff()) {
            // no particle has a positive weight: log p^ = -inf, the particles stay as they are
            loglik = mx;
            if (j == 0) {
                q.incr[mk] = mx; q.ess[mk] = 0.f;
                for (int i = 0; i < S; ++i) q.mean[mk * S + i] = q.std[mk * S + i] = __builtin_nanf("");
            }
            if (q.ancestors) q.ancestors[mk * N + j] = j;
            continue;
        }
        const float wt = expf(lw - mx);
        // inclusive scan of the weights: Hillis-Steele in the wave, then a running maximum (pf_kernel has the reason)
        float cs = wt;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const float tt = __shfl_up(cs, off, 64);
            if (lane >= off) cs += tt;
        }
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const float tt = __shfl_up(cs, off, 64);
            if (lane >= off) cs = fmaxf(cs, tt);
        }
        if (lane == kWave - 1) red[wave] = cs;
        __syncthreads();
        float base = 0.f, total = 0.f;
        for (int w2 = 0; w2 < nwaves; ++w2) {
            if (w2 == wave) base = total;
            total += red[w2];
        }
        __syncthreads();
        cs += base;
        // sum w^2 and sum w x, then sum w (x - mean)^2: two passes, four dims per reduction round
        constexpr int CH = S < 4 ? S : 4;
        float mean[S], s2 = 0.f;
#pragma unroll
        for (int i0 = 0; i0 < S; i0 += CH) {
            float v[CH + 1];
            v[0] = wt * wt;
#pragma unroll
            for (int i = 0; i < CH; ++i) v[1 + i] = (i0 + i < S && wt > 0.f) ? wt * xf[i0 + i < S ? i0 + i : 0] : 0.f;
            pf_block_sum<CH + 1>(v, red, lane, wave, nwaves);
            s2 = v[0];
#pragma unroll
            for (int i = 0; i < CH; ++i)
                if (i0 + i < S) mean[i0 + i] = v[1 + i] / total;
        }
#pragma unroll
        for (int i0 = 0; i0 < S; i0 += CH) {
            float d[CH];
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const int ii = i0 + i < S ? i0 + i : 0;
                const float dx = xf[ii] - mean[ii];
                d[i] = (i0 + i < S && wt > 0.f) ? wt * dx * dx : 0.f;
            }
            pf_block_sum<CH>(d, red, lane, wave, nwaves);
            if (j == 0)
#pragma unroll
                for (int i = 0; i < CH; ++i)
                    if (i0 + i < S) { q.mean[mk * S + i0 + i] = mean[i0 + i]; q.std[mk * S + i0 + i] = sqrtf(d[i] / total); }
        }
        const float inc = mx + logf(total) - q.log_n;
        loglik += inc;
        if (j == 0) { q.incr[mk] = inc; q.ess[mk] = total * total / s2; }
        // systematic resampling: ancestor_j = min(#{i : C_i <= (j + u) / N C_{N-1}}, N - 1); the rows hold the int32 state
        cum[j] = cs;
#pragma unroll
        for (int i = 0; i < S; ++i) rows_s[j * RS + i] = x[i];
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
        for (int i = 0; i < S; ++i) x[i] = rows_s[anc * RS + i];
        if (q.ancestors) q.ancestors[mk * N + j] = anc;
        __syncthreads();
    }
    if (j == 0) p.loglik[m] = loglik;
}

// One body for the two entry points.  Every check, the descriptors' included, comes before the first HIP call.
static int jump_particle_filter(const SdeRoute &rt, int M, int N, int S, int P, int K, int O, const int32_t *x0, const float *theta,
                                const double *obs_times, const float *obs_values, const float *obs_matrix, int lik_kind,
                                double variance, double scale, double dispersion, const float *row_const, const uint32_t *key,
                                int max_events, float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                float *filtered_std, int32_t *stopped, float *mean_events, int32_t *particles, int *ancestors,
                                float *log_weights, int32_t *events, void *stream) {
    JfParams p = {};
    const int rc = crn_route_net(rt, S, P, p.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(M >= 1 && K >= 1, VSDE_E_BADARG, "bad jump particle-filter dims M=%d K=%d", M, K);
    VSDE_CHECK_ARG(N >= kWave && N <= kPfMaxN && N % kWave == 0, VSDE_E_BADARG,
                   "jump particle filter: %d particles (a multiple of %d up to %d supported)", N, kWave, kPfMaxN);
    VSDE_CHECK_ARG((int64_t)M * N < ((int64_t)1 << 32), VSDE_E_BADARG, "jump particle filter: M N = %lld paths (below 2^32 supported)",
                   (long long)M * N);
    VSDE_CHECK_ARG(O >= 1 && O <= kPfMaxO, VSDE_E_BADARG, "jump particle filter: obs_dim %d (1..%d supported)", O, kPfMaxO);
    VSDE_CHECK_ARG(obs_matrix || O == S, VSDE_E_BADARG, "without an observation matrix obs_dim must equal state_dim (%d vs %d)", O, S);
    VSDE_CHECK_ARG(max_events >= 1 && max_events <= kJfMaxEvents, VSDE_E_BADARG, "jump particle filter: max_events %d outside 1..%d",
                   max_events, kJfMaxEvents);
    VSDE_CHECK_ARG(lik_kind == VSDE_LIK_GAUSSIAN || lik_kind == VSDE_LIK_POISSON || lik_kind == VSDE_LIK_NEGATIVE_BINOMIAL, VSDE_E_BADARG,
                   "unknown likelihood %d (0 = Gaussian, 1 = Poisson, 2 = negative binomial)", lik_kind);
    if (lik_kind == VSDE_LIK_GAUSSIAN) {
        VSDE_CHECK_ARG(variance > 0, VSDE_E_BADARG, "jump particle filter: the variance must be positive");
        p.inv_var = (float)(1.0 / variance); p.log_norm = (float)(-0.5 * log(2.0 * M_PI * variance));
    } else {
        const int rc2 = count_lik(p.cl, lik_kind, scale, dispersion, row_const, K);
        if (rc2) return rc2;
    }
    VSDE_CHECK_ARG(x0 && theta && obs_times && obs_values && key && log_likelihood && increments && ess && filtered_mean &&
                   filtered_std && stopped && mean_events, VSDE_E_BADARG, "jump particle filter: NULL argument");
    p.M = M; p.N = N; p.S = S; p.P = P; p.K = K; p.O = O; p.max_events = max_events; p.lik = lik_kind;
    p.x0 = x0; p.theta = theta; p.times = obs_times; p.obs_values = obs_values; p.obs_matrix = obs_matrix; p.key = key;
    p.loglik = log_likelihood; p.incr = increments; p.ess = ess; p.mean = filtered_mean; p.std = filtered_std;
    p.mean_events = mean_events; p.stopped = stopped; p.particles = particles; p.ancestors = ancestors; p.log_weights = log_weights;
    p.events = events; p.log_n = (float)log((double)N);
    for (int j = 0; j < p.net.R; ++j) {
        p.orders[j] = crn_pack_orders(rt.net, j);
        for (int i = 0; i < S; ++i) p.nu[j][i >> 2] |= (uint32_t)(uint8_t)rt.net->change[j][i] << (8 * (i & 3));
    }
    const size_t lds = ((size_t)N * ((S | 1) + 1) + kPfRed) * sizeof(float);   // at most 41 KiB: below the 64 KiB default
    const auto launch = [&](auto kern, int max_n) {
        VSDE_CHECK_ARG(N <= max_n, VSDE_E_BADARG, "jump particle filter: %d particles (up to %d supported for this network)", N, max_n);
        hipLaunchKernelGGL(kern, dim3(M), dim3(N), lds, (hipStream_t)stream, p);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    };
    return crn_dispatch(S, p.net.R, [&](auto ns, auto nr) {
        constexpr int NS = decltype(ns)::value, NR = decltype(nr)::value;
        if (rt.descriptors == 2) return launch(jf_kernel<NS, NR, true>, jf_max_n(NS, NR, true));
        return launch(jf_kernel<NS, NR, false>, jf_max_n(NS, NR, false));
    });
}

}  // namespace vsde

using namespace vsde;

extern "C" int vsde_crn_jump_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const int32_t *x0,
                                             const float *theta, const double *obs_times, const float *obs_values,
                                             const float *obs_matrix, int lik_kind, double variance, double scale, double dispersion,
                                             const float *row_const, const uint32_t *key, int max_events, float *log_likelihood,
                                             float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                             int32_t *stopped, float *mean_events, int32_t *particles, int *ancestors,
                                             float *log_weights, int32_t *events, void *stream) {
    return jump_particle_filter(crn_route(net), M, N, S, P, K, O, x0, theta, obs_times, obs_values, obs_matrix, lik_kind, variance,
                                scale, dispersion, row_const, key, max_events, log_likelihood, increments, ess, filtered_mean,
                                filtered_std, stopped, mean_events, particles, ancestors, log_weights, events, stream);
}

extern "C" int vsde_crn_kinetic_jump_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                     int P, int K, int O, const int32_t *x0, const float *rates,
                                                     const double *obs_times, const float *obs_values, const float *obs_matrix,
                                                     int lik_kind, double variance, double scale, double dispersion,
                                                     const float *row_const, const uint32_t *key, int max_events,
                                                     float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                                     float *filtered_std, int32_t *stopped, float *mean_events, int32_t *particles,
                                                     int *ancestors, float *log_weights, int32_t *events, void *stream) {
    return jump_particle_filter(crn_route(net, kin), M, N, S, P, K, O, x0, rates, obs_times, obs_values, obs_matrix, lik_kind, variance,
                                scale, dispersion, row_const, key, max_events, log_likelihood, increments, ess, filtered_mean,
                                filtered_std, stopped, mean_events, particles, ancestors, log_weights, events, stream);
}
