// Tau-leaping for the jump process of a reaction network (gfx950): a fixed step tau with Poisson-many firings of every reaction on
// an integer state, as a simulator (tl_kernel) and as the propagator of a bootstrap particle filter (tlf_kernel).
// viforsdes_amd/core/tau_leap.py and viforsdes_amd/inference/tau_leap_filter.py are the specification.
//
// Step t of path b from the state x (tl_step):
//   a_j = crn_jump_propensity (fp32); a NaN, infinite or negative a_j                      -> stopped (status 2)
//   lam_j = a_j * (float)tau, one fp32 product, then widened to float64; lam_j > 2^30        -> stopped
//   n_j = poisson_draw(lam_j, {t, j, b}) (vsde_poisson.h), every draw on the propensities at the start of the step; a failed draw
//                                                                                           -> stopped
//   in reaction order on the running state (int64): n_j <- min(n_j, min over the species with r_ji > 0 of x_i / r_ji) (a reduced
//   n_j counts as capped), x <- x + n_j nu_j; any x_i > 2^30 after the last reaction         -> stopped
// A stopped path keeps the state from before the step, and the step adds nothing to its capped count.
//
// The propensities of all reactions are formed first (unrolled to the bound NR: th and lam stay in registers); the draws and the
// updates then run in ONE run-time loop over j, so the float64 sampler exists once per kernel, not NR times: lam_j is picked by
// compare-selects over the registers and the reaction's rows are uniform loads from the argument block.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vsde_filter_kernels.h"
#include "vsde_poisson.h"

namespace vsde {

constexpr float kTlMaxRate = 1073741824.f;          // 2^30
constexpr long long kTlMaxCopy = 1073741824ll;      // 2^30

struct TlTables {
    uint32_t orders[kCrnMaxR];   // reactant row of reaction j, 2 bits per species (crn_pack_orders)
    uint32_t nu[kCrnMaxR][2];    // net change of reaction j, one int8 per species: species 0..3, 4..7
    CrnNet net;                  // R and the rate-law tables
};

static inline void tl_tables(TlTables &tb, const SdeRoute &rt, int S) {
    for (int j = 0; j < tb.net.R; ++j) {
        tb.orders[j] = crn_pack_orders(rt.net, j);
        for (int i = 0; i < S; ++i) tb.nu[j][i >> 2] |= (uint32_t)(uint8_t)rt.net->change[j][i] << (8 * (i & 3));
    }
}

// one step; 0: x is the new state and `capped` has grown by the reduced draws; 2: stopped, x and capped unchanged.  log: the R raw
// draws of the step are written there (NULL: not logged); the caller overwrites the row of a stopped step
template <int S, int NR, bool KIN>
__device__ __forceinline__ int tl_step(const TlTables &tb, int (&x)[S], const float *th, float tau, uint32_t t, uint32_t b,
                                       uint32_t k0, uint32_t k1, int32_t *log, int &capped) {
    const int R = tb.net.R;
    float xf[S], lam[NR];
#pragma unroll
    for (int i = 0; i < S; ++i) xf[i] = (float)x[i];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        lam[j] = 0.f;
        if (j < R) {
            const float a = crn_jump_propensity<S, NR, KIN>(tb.net, tb.orders[j], j, x, xf, th);
            lam[j] = a * tau;
            bad = bad || !(a >= 0.f) || a == INFINITY || lam[j] > kTlMaxRate;
        }
    }
    if (bad) return 2;
    long long xr[S];
#pragma unroll
    for (int i = 0; i < S; ++i) xr[i] = x[i];
    int reduced = 0;
#pragma unroll 1
    for (int j = 0; j < R; ++j) {
        float lj = 0.f;
#pragma unroll
        for (int jj = 0; jj < NR; ++jj)
            if (jj == j) lj = lam[jj];
        const int n = poisson_draw((double)lj, t, (uint32_t)j, b, k0, k1);
        if (log) log[j] = n;
        if (n < 0) return 2;
        const uint32_t ord = tb.orders[j], lo = tb.nu[j][0], hi = S > 4 ? tb.nu[j][1] : 0u;
        long long m = n;
#pragma unroll
        for (int i = 0; i < S; ++i) {
            const uint32_t r = (ord >> (2 * i)) & 3u;
            const long long q = r == 3u ? xr[i] / 3 : r == 2u ? xr[i] >> 1 : xr[i];
            if (r != 0u && q < m) m = q;
        }
        if (m < (long long)n) ++reduced;
#pragma unroll
        for (int i = 0; i < S; ++i) xr[i] += m * (long long)(int8_t)((i < 4 ? lo : hi) >> (8 * (i & 3)));
    }
    bool over = false;
#pragma unroll
    for (int i = 0; i < S; ++i) over = over || xr[i] > kTlMaxCopy;
    if (over) return 2;
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = (int)xr[i];
    capped += reduced;
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The simulator: a thread per trajectory, 64-thread workgroups; x, the constants and the draws live in registers, memory traffic
// is x0, theta, the key and the rows in, the requested rows (and the optional draw log) out.
struct TlParams {
    int B, K, E, P;
    float tau;
    const int32_t *x0;       // [B][S]
    const float *theta;      // [B][P]: k (P = R), or the effective constants (k, K) (P = 2R)
    const int32_t *rows;     // [K] non-decreasing grid rows: row r is read after steps 0 .. r - 1
    const uint32_t *key;     // 2 words
    int32_t *states;         // [B][K][S]
    int32_t *status, *capped;   // [B]
    int32_t *draws;          // [B][E][R] or NULL
    TlTables tb;
};

template <int S, int NR, bool KIN> __global__ void __launch_bounds__(64) tl_kernel(TlParams p) {
    constexpr int P = KIN ? 2 * NR : NR;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int R = p.tb.net.R;
    const uint32_t k0 = p.key[0], k1 = p.key[1];
    int x[S];
    float th[P];
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = p.x0[(int64_t)b * S + i];
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, R, true);
    else em_load_theta<4, P>(th, p.theta, b, p.P, true);
    int32_t *out = p.states + (int64_t)b * p.K * S;
    int32_t *log = p.E > 0 ? p.draws + (int64_t)b * p.E * R : nullptr;
    int t = 0, k = 0, st = 0, capped = 0;
#pragma unroll 1
    for (; k < p.K; ++k) {
        const int row = p.rows[k];
#pragma unroll 1
        while (t < row) {
            st = tl_step<S, NR, KIN>(p.tb, x, th, p.tau, (uint32_t)t, (uint32_t)b, k0, k1, t < p.E ? log + (int64_t)t * R : nullptr,
                                     capped);
            if (st != 0) break;
            ++t;
        }
        if (st != 0) break;
#pragma unroll
        for (int i = 0; i < S; ++i) out[(int64_t)k * S + i] = x[i];
    }
    for (; k < p.K; ++k) {
#pragma unroll
        for (int i = 0; i < S; ++i) out[(int64_t)k * S + i] = -1;
    }
    // the step the path stopped at (its row may be half written) and every step it never took
    for (int e = t; e < p.E; ++e)
        for (int j = 0; j < R; ++j) log[(int64_t)e * R + j] = -1;
    p.status[b] = st;
    p.capped[b] = capped;
}

// every check, the descriptors' included, comes before the first HIP call
static int tau_leap_process(const SdeRoute &rt, int B, int S, int P, int K, int E, const int32_t *x0, const float *theta,
                            const int32_t *out_rows, const uint32_t *key, double time_step, int32_t *states, int32_t *status,
                            int32_t *capped, int32_t *draws, void *stream) {
    TlParams p = {};
    const int rc = crn_route_net(rt, S, P, p.tb.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(B >= 1 && K >= 1 && E >= 0, VSDE_E_BADARG, "bad tau-leap dims B=%d K=%d E=%d", B, K, E);
    VSDE_CHECK_ARG(time_step > 0 && std::isfinite(time_step), VSDE_E_BADARG, "tau-leap: the time step must be positive and finite");
    VSDE_CHECK_ARG(x0 && theta && out_rows && key && states && status && capped, VSDE_E_BADARG, "tau-leap: NULL argument");
    VSDE_CHECK_ARG(E == 0 || draws, VSDE_E_BADARG, "tau-leap: E=%d steps to log but a NULL log pointer", E);
    p.B = B; p.K = K; p.E = E; p.P = P; p.tau = (float)time_step;
    tl_tables(p.tb, rt, S);
    p.x0 = x0; p.theta = theta; p.rows = out_rows; p.key = key;
    p.states = states; p.status = status; p.capped = capped; p.draws = draws;
    const dim3 grid((unsigned)((B + 63) / 64)), block(64);
    return crn_dispatch(S, p.tb.net.R, [&](auto ns, auto nr) {
        constexpr int NS = decltype(ns)::value, NR = decltype(nr)::value;
        if (rt.descriptors == 2) hipLaunchKernelGGL((tl_kernel<NS, NR, true>), grid, block, 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((tl_kernel<NS, NR, false>), grid, block, 0, (hipStream_t)stream, p);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    });
}

// ---------------------------------------------------------------------------------------------------------------------
// The filter: a workgroup per theta, a thread per particle (N a multiple of 64), jf_kernel's layout (vsde_jump_filter.hip): the
// int32 state, the constants and the running log-likelihood in registers, the int32 bits of the state in the LDS rows that
// resampling gathers.  Segment k runs steps rows[k-1] .. rows[k] - 1 (rows[-1] = 0) of particle slot j of filter m as path
// b = m N + j: a slot keeps its stream across resampling.  A stopped particle keeps its state, weighs -inf at observation k and
// carries on from that state at the next segment only if the whole filter is dead.  Observation k is jf_kernel's stage, operation
// for operation: log-weight on (float)x, wave max, Hillis-Steele scan plus running maximum, wave totals through LDS, two-pass
// moments four dims per round, binary search over the cumulative sums.
// LDS (dynamic): N cumulative sums + N (S | 1) state words + 16 x 18 reduction slots: 41 KiB at N = 1024, S = 8.

// Particles per filter an instantiation is built for (_hip.tau_leap_filter_max_particles restates it): the float64 sampler needs
// more than the 128 VGPRs a lane has in a 1024-thread workgroup, 512 threads leave 256.
constexpr int tlf_max_n(int S, int NR, bool kin) { return kPfMaxN / 2; }

struct TlfParams {
    int M, N, S, P, K, O, lik;   // lik: VSDE_LIK_GAUSSIAN / POISSON / NEGATIVE_BINOMIAL
    float tau;
    const int32_t *x0;         // [M][S]
    const float *theta;        // [M][P]
    const int32_t *rows;       // [K] non-decreasing grid rows of the observations
    const float *obs_values;   // [K][O]
    const float *obs_matrix;   // [O][S] or NULL (O == S)
    const uint32_t *key;       // 2 words
    float *loglik, *incr, *ess, *mean, *std;
    int32_t *stopped, *capped;   // [M][K]
    int32_t *particles;        // [M][K][N][S] or NULL
    int *ancestors;            // [M][K][N] or NULL
    float *log_weights;        // [M][K][N] or NULL
    float inv_var, log_norm, log_n;
    CountLik cl;
    TlTables tb;
};

// The kernel's argument block through a pointer the compiler cannot see through (jf_args_again, vsde_jump_filter.hip): loads from it
// stay where they are written, at the observations, instead of being hoisted above the step loop as loop-invariant SGPRs that are
// then spilled around every segment.  The block is the kernel's only argument: offset 0 of the segment
__device__ __forceinline__ const TlfParams &tlf_args_again() {
    uint64_t a = (uint64_t)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return *(const TlfParams *)(const __attribute__((address_space(4))) void *)a;
}

template <int S, int NR, bool KIN> __global__ void __launch_bounds__(tlf_max_n(S, NR, KIN)) tlf_kernel(TlfParams p) {
    constexpr int P = KIN ? 2 * NR : NR, RS = S | 1;
    extern __shared__ __attribute__((aligned(16))) float tlf_lds[];
    const int N = p.N, R = p.tb.net.R;
    float *cum = tlf_lds, *red = cum + N + N * RS;
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
    int t = 0;
#pragma unroll 1
    for (int k = 0; k < p.K; ++k) {
        // ---- the segment: steps t .. rows[k] - 1
        const int row = p.rows[k];
        int st = 0, ncap = 0;
#pragma unroll 1
        for (; t < row; ++t) {
            st = tl_step<S, NR, KIN>(p.tb, x, th, p.tau, (uint32_t)t, b, k0, k1, nullptr, ncap);
            if (st != 0) break;
        }
        t = row;
        // ---- observation k: jf_kernel's stage on (float)x; a stopped particle weighs -inf.  Its arguments are read again here
        // (tlf_args_again): hoisted out of both loops they would crowd the step's tables out of the SGPRs
        const TlfParams &q = tlf_args_again();
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
        if (q.particles)
#pragma unroll
            for (int i = 0; i < S; ++i) q.particles[(mk * N + j) * S + i] = x[i];
        {
            // the segment's record: stopped particles and capped draws (exact in fp32 up to 2^24)
            float v[2] = {st != 0 ? 1.f : 0.f, (float)ncap};
            pf_block_sum<2>(v, red, lane, wave, nwaves);
            if (j == 0) { q.stopped[mk] = (int32_t)v[0]; q.capped[mk] = (int32_t)v[1]; }
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
        const float thr = ((float)j + u) / (float)N * total;
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cum[mid] <= thr) lo = mid + 1;
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
static int tau_leap_particle_filter(const SdeRoute &rt, int M, int N, int S, int P, int K, int O, const int32_t *x0, const float *theta,
                                    const int32_t *obs_rows, const float *obs_values, const float *obs_matrix, int lik_kind,
                                    double variance, double scale, double dispersion, const float *row_const, const uint32_t *key,
                                    double time_step, float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                    float *filtered_std, int32_t *stopped, int32_t *capped, int32_t *particles, int *ancestors,
                                    float *log_weights, void *stream) {
    TlfParams p = {};
    const int rc = crn_route_net(rt, S, P, p.tb.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(M >= 1 && K >= 1, VSDE_E_BADARG, "bad tau-leap particle-filter dims M=%d K=%d", M, K);
    VSDE_CHECK_ARG(N >= kWave && N <= kPfMaxN && N % kWave == 0, VSDE_E_BADARG,
                   "tau-leap particle filter: %d particles (a multiple of %d up to %d supported)", N, kWave, kPfMaxN);
    VSDE_CHECK_ARG((int64_t)M * N < ((int64_t)1 << 32), VSDE_E_BADARG, "tau-leap particle filter: M N = %lld paths (below 2^32 supported)",
                   (long long)M * N);
    VSDE_CHECK_ARG(O >= 1 && O <= kPfMaxO, VSDE_E_BADARG, "tau-leap particle filter: obs_dim %d (1..%d supported)", O, kPfMaxO);
    VSDE_CHECK_ARG(obs_matrix || O == S, VSDE_E_BADARG, "without an observation matrix obs_dim must equal state_dim (%d vs %d)", O, S);
    VSDE_CHECK_ARG(time_step > 0 && std::isfinite(time_step), VSDE_E_BADARG,
                   "tau-leap particle filter: the time step must be positive and finite");
    VSDE_CHECK_ARG(lik_kind == VSDE_LIK_GAUSSIAN || lik_kind == VSDE_LIK_POISSON || lik_kind == VSDE_LIK_NEGATIVE_BINOMIAL, VSDE_E_BADARG,
                   "unknown likelihood %d (0 = Gaussian, 1 = Poisson, 2 = negative binomial)", lik_kind);
    if (lik_kind == VSDE_LIK_GAUSSIAN) {
        VSDE_CHECK_ARG(variance > 0, VSDE_E_BADARG, "tau-leap particle filter: the variance must be positive");
        p.inv_var = (float)(1.0 / variance); p.log_norm = (float)(-0.5 * log(2.0 * M_PI * variance));
    } else {
        const int rc2 = count_lik(p.cl, lik_kind, scale, dispersion, row_const, K);
        if (rc2) return rc2;
    }
    VSDE_CHECK_ARG(x0 && theta && obs_rows && obs_values && key && log_likelihood && increments && ess && filtered_mean &&
                   filtered_std && stopped && capped, VSDE_E_BADARG, "tau-leap particle filter: NULL argument");
    p.M = M; p.N = N; p.S = S; p.P = P; p.K = K; p.O = O; p.lik = lik_kind; p.tau = (float)time_step;
    p.x0 = x0; p.theta = theta; p.rows = obs_rows; p.obs_values = obs_values; p.obs_matrix = obs_matrix; p.key = key;
    p.loglik = log_likelihood; p.incr = increments; p.ess = ess; p.mean = filtered_mean; p.std = filtered_std;
    p.stopped = stopped; p.capped = capped; p.particles = particles; p.ancestors = ancestors; p.log_weights = log_weights;
    p.log_n = (float)log((double)N);
    tl_tables(p.tb, rt, S);
    const size_t lds = ((size_t)N * ((S | 1) + 1) + kPfRed) * sizeof(float);   // at most 41 KiB: below the 64 KiB default
    const auto launch = [&](auto kern, int max_n) {
        VSDE_CHECK_ARG(N <= max_n, VSDE_E_BADARG, "tau-leap particle filter: %d particles (up to %d supported for this network)", N, max_n);
        hipLaunchKernelGGL(kern, dim3(M), dim3(N), lds, (hipStream_t)stream, p);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    };
    return crn_dispatch(S, p.tb.net.R, [&](auto ns, auto nr) {
        constexpr int NS = decltype(ns)::value, NR = decltype(nr)::value;
        if (rt.descriptors == 2) return launch(tlf_kernel<NS, NR, true>, tlf_max_n(NS, NR, true));
        return launch(tlf_kernel<NS, NR, false>, tlf_max_n(NS, NR, false));
    });
}

}  // namespace vsde

using namespace vsde;

extern "C" int vsde_crn_tau_leap_process(const vsde_crn_network *net, int B, int S, int P, int K, int E, const int32_t *x0,
                                         const float *theta, const int32_t *out_rows, const uint32_t *key, double time_step,
                                         int32_t *states, int32_t *status, int32_t *capped, int32_t *draws, void *stream) {
    return tau_leap_process(crn_route(net), B, S, P, K, E, x0, theta, out_rows, key, time_step, states, status, capped, draws, stream);
}

extern "C" int vsde_crn_kinetic_tau_leap_process(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K,
                                                 int E, const int32_t *x0, const float *rates, const int32_t *out_rows,
                                                 const uint32_t *key, double time_step, int32_t *states, int32_t *status,
                                                 int32_t *capped, int32_t *draws, void *stream) {
    return tau_leap_process(crn_route(net, kin), B, S, P, K, E, x0, rates, out_rows, key, time_step, states, status, capped, draws,
                            stream);
}

extern "C" int vsde_crn_tau_leap_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O,
                                                 const int32_t *x0, const float *theta, const int32_t *obs_rows,
                                                 const float *obs_values, const float *obs_matrix, int lik_kind, double variance,
                                                 double scale, double dispersion, const float *row_const, const uint32_t *key,
                                                 double time_step, float *log_likelihood, float *increments, float *ess,
                                                 float *filtered_mean, float *filtered_std, int32_t *stopped, int32_t *capped,
                                                 int32_t *particles, int *ancestors, float *log_weights, void *stream) {
    return tau_leap_particle_filter(crn_route(net), M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, lik_kind, variance,
                                    scale, dispersion, row_const, key, time_step, log_likelihood, increments, ess, filtered_mean,
                                    filtered_std, stopped, capped, particles, ancestors, log_weights, stream);
}

extern "C" int vsde_crn_kinetic_tau_leap_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                         int P, int K, int O, const int32_t *x0, const float *rates,
                                                         const int32_t *obs_rows, const float *obs_values, const float *obs_matrix,
                                                         int lik_kind, double variance, double scale, double dispersion,
                                                         const float *row_const, const uint32_t *key, double time_step,
                                                         float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                                         float *filtered_std, int32_t *stopped, int32_t *capped, int32_t *particles,
                                                         int *ancestors, float *log_weights, void *stream) {
    return tau_leap_particle_filter(crn_route(net, kin), M, N, S, P, K, O, x0, rates, obs_rows, obs_values, obs_matrix, lik_kind,
                                    variance, scale, dispersion, row_const, key, time_step, log_likelihood, increments, ess,
                                    filtered_mean, filtered_std, stopped, capped, particles, ancestors, log_weights, stream);
}
