// Metropolis step of particle marginal Metropolis-Hastings (gfx950): everything of a PMMH iteration that is not the particle filter
// (viforsdes_amd/inference/particle_mcmc.py is the specification).  One launch, a thread per chain, CLOSES iteration `iteration - 1`
// (log-mean-exp of the chain's R filter estimates, the acceptance rule, the state update, the optional store of the kept row, the
// acceptance counter) and OPENS iteration `iteration` (Philox normals, u' = u + step L z, theta', log prior + Jacobian, R copies of
// theta' for the filter launch, the filter key of the iteration).  The chain's u stays in registers between the two halves.
// P is a template argument: u, z and theta' are register arrays under fully unrolled loops (a run-time P <= 16 bound would index
// them dynamically and put them into scratch), and the lower triangle of L is addressed by compile-time offsets.  L, the prior
// constants and the mask travel by value in the kernel argument block: every lane reads them at the same address (scalar loads),
// and the host checks L before any HIP call.  Plain vector stores only; n_accept[c] belongs to thread c.
// PATHS (vsde_pmmh_step_paths): the chain also carries one latent path of its current point as a record (anchors, noise paths,
// iteration).  The thread of an ACCEPTED chain draws the proposal's record from what the closed iteration's filters stored: a filter
// in proportion to its estimate, a uniformly chosen offspring slot of the last resampling, its lineage through `ancestors` (K
// dependent loads, every entry clamped into its row) and the particles on it.  The PATHS = false instantiations are the code they were.
#include "vsde_sde_step.h"

namespace vsde {

constexpr int kMcMaxP = 16, kMcThreads = 64;

struct McParams {
    int C, R, iteration;
    uint32_t pos_mask;
    int prior_lognormal;
    float prior_mean, prior_inv_std, prior_const;   // const = -log(std) - 0.5 log(2 pi)
    float step, log_r;
    const uint32_t *key;
    const float *loglik_prop;
    float *cur_u, *cur_target, *cur_loglik, *prop_u, *prop_lp, *theta_prop;
    uint32_t *filter_key;
    float *sample_row, *loglik_row, *target_row;
    int *n_accept;
    float L[kMcMaxP * kMcMaxP];                     // row-major [P][P], the lower triangle is read
};

// the record half of vsde_pmmh_step_paths: what the closed iteration's filter launch stored, the chains' records, the optional rows
struct McPaths {
    int N, K, S;
    const float *particles;                         // [C R][K][N][S]
    const int *ancestors;                           // [C R][K][N]
    float *cur_anchor;                              // [C][K][S]
    uint32_t *cur_noise;                            // [C][K]
    int *cur_iter;                                  // [C]
    float *anchor_row;
    uint32_t *noise_row;
    int *iter_row;
};

constexpr uint32_t kMcDeadPath = 0xFFFFFFFFu;

template <int P, bool PATHS>
__global__ __launch_bounds__(kMcThreads) void pmmh_step_kernel(const McParams p, const McPaths q) {
    const int c = blockIdx.x * kMcThreads + threadIdx.x;
    const uint32_t k0 = p.key[0], k1 = p.key[1];
    if (c == 0) {
        const uint4 w = philox4x32_10(make_uint4((uint32_t)p.iteration, 0u, 0u, 5u), k0, k1);
        p.filter_key[0] = w.x; p.filter_key[1] = w.y;
    }
    if (c >= p.C) return;
    const int64_t row = (int64_t)c * P;
    float u[P];
#pragma unroll
    for (int j = 0; j < P; ++j) u[j] = p.cur_u[row + j];

    if (p.loglik_prop) {                            // close iteration `iteration - 1`
        const float *l = p.loglik_prop + (int64_t)c * p.R;
        float mx = -INFINITY;
        bool nan = false;
        for (int r = 0; r < p.R; ++r) { const float v = l[r]; nan |= v != v; mx = fmaxf(mx, v); }
        float ll;
        if (nan) ll = NAN;
        else if (mx == -INFINITY) ll = -INFINITY;
        else {
            float s = 0.f;
            for (int r = 0; r < p.R; ++r) s += expf(l[r] - mx);
            ll = mx + logf(s) - p.log_r;
        }
        const float tp = p.prop_lp[c] + ll;
        float tc = p.cur_target[c], lc = p.cur_loglik[c];
        const int it = p.iteration - 1;
        const uint4 w = philox4x32_10(make_uint4((uint32_t)it, 0u, (uint32_t)c, 4u), k0, k1);
        const float log_u = logf(philox_uniform(w.x));
        const bool accept = tp == tp && (it == 0 || (tp != -INFINITY && log_u < tp - tc));
        if (accept) {
#pragma unroll
            for (int j = 0; j < P; ++j) { u[j] = p.prop_u[row + j]; p.cur_u[row + j] = u[j]; }
            tc = tp; lc = ll;
            p.cur_target[c] = tc; p.cur_loglik[c] = lc;
            p.n_accept[c] += 1;
        }
        if constexpr (PATHS) {
            const int64_t ck = (int64_t)c * q.K;
            if (accept) {
                if (!(mx > -INFINITY)) {            // every filter died (iteration 0 accepts it): a dead record
                    for (int k = 0; k < q.K; ++k) {
                        q.cur_noise[ck + k] = kMcDeadPath;
                        for (int i = 0; i < q.S; ++i) q.cur_anchor[(ck + k) * q.S + i] = NAN;
                    }
                } else {
                    const uint4 w6 = philox4x32_10(make_uint4((uint32_t)it, 0u, (uint32_t)c, 6u), k0, k1);
                    // the filter, in proportion to its estimate: sums in r order never decrease, so they are their running maximum
                    float total = 0.f;
                    for (int r = 0; r < p.R; ++r) total += expf(l[r] - mx);
                    const float tau = philox_uniform(w6.x) * total;
                    float cum = 0.f;
                    int rs = 0;
                    for (int r = 0; r < p.R; ++r) { cum += expf(l[r] - mx); rs += cum <= tau; }
                    rs = min(rs, p.R - 1);
                    const int N = q.N, m = c * p.R + rs;
                    // a uniformly chosen offspring slot of the last resampling: its ancestor is a draw from the final weights
                    const int J = min((int)floorf(philox_uniform(w6.y) * (float)N), N - 1);
                    const int *anc = q.ancestors + (int64_t)m * q.K * N;
                    int slot = min(max(anc[(int64_t)(q.K - 1) * N + J], 0), N - 1);
                    for (int k = q.K - 1; k >= 0; --k) {
                        q.cur_noise[ck + k] = (uint32_t)m * (uint32_t)N + (uint32_t)slot;
                        const float *x = q.particles + (((int64_t)m * q.K + k) * N + slot) * q.S;
                        for (int i = 0; i < q.S; ++i) q.cur_anchor[(ck + k) * q.S + i] = x[i];
                        if (k > 0) slot = min(max(anc[(int64_t)(k - 1) * N + slot], 0), N - 1);
                    }
                }
                q.cur_iter[c] = it;
            }
            // the thread reads back what it alone wrote
            if (q.anchor_row)
                for (int64_t e = ck * q.S; e < (ck + q.K) * q.S; ++e) q.anchor_row[e] = q.cur_anchor[e];
            if (q.noise_row)
                for (int k = 0; k < q.K; ++k) q.noise_row[ck + k] = q.cur_noise[ck + k];
            if (q.iter_row) q.iter_row[c] = q.cur_iter[c];
        }
        if (p.sample_row) {
#pragma unroll
            for (int j = 0; j < P; ++j) p.sample_row[row + j] = ((p.pos_mask >> j) & 1u) ? expf(u[j]) : u[j];
        }
        if (p.loglik_row) p.loglik_row[c] = lc;
        if (p.target_row) p.target_row[c] = tc;
    }

    // open iteration `iteration`: iteration 0 proposes what the caller put into prop_u
    if (p.iteration > 0) {
        float z[(P + 3) / 4 * 4];
#pragma unroll
        for (int b = 0; b < (P + 3) / 4; ++b) {
            const uint4 w = philox4x32_10(make_uint4((uint32_t)p.iteration, (uint32_t)b, (uint32_t)c, 3u), k0, k1);
            box_muller(w.x, w.y, z[4 * b], z[4 * b + 1]);
            box_muller(w.z, w.w, z[4 * b + 2], z[4 * b + 3]);
        }
#pragma unroll
        for (int i = 0; i < P; ++i) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j <= i; ++j) s += p.L[i * P + j] * z[j];
            u[i] += p.step * s;
            p.prop_u[row + i] = u[i];
        }
    } else {
#pragma unroll
        for (int j = 0; j < P; ++j) u[j] = p.prop_u[row + j];
    }
    float th[P], lp = 0.f;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const bool pos = (p.pos_mask >> j) & 1u;
        th[j] = pos ? expf(u[j]) : u[j];
        const float lg = pos ? u[j] : (p.prior_lognormal ? logf(th[j]) : 0.f);
        const float zp = ((p.prior_lognormal ? lg : th[j]) - p.prior_mean) * p.prior_inv_std;
        lp += -0.5f * zp * zp + p.prior_const - (p.prior_lognormal ? lg : 0.f) + (pos ? u[j] : 0.f);
    }
    p.prop_lp[c] = lp;
    for (int r = 0; r < p.R; ++r) {
        float *t = p.theta_prop + ((int64_t)c * p.R + r) * P;
#pragma unroll
        for (int j = 0; j < P; ++j) t[j] = th[j];
    }
}

template <int P, bool PATHS>
static int pmmh_launch(const McParams &p, const McPaths &q, void *stream) {
    hipLaunchKernelGGL((pmmh_step_kernel<P, PATHS>), dim3((unsigned)((p.C + kMcThreads - 1) / kMcThreads)), dim3(kMcThreads), 0,
                       (hipStream_t)stream, p, q);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}


// One body for vsde_pmmh_step (paths = nullptr) and vsde_pmmh_step_paths.  Every check comes before the first HIP call.
static int pmmh_step(const McPaths *paths, int C, int P, int R, int iteration, const float *scale_tril, double step_size, int prior_type,
                     double prior_mean, double prior_std, const uint8_t *theta_positive_mask_host, const uint32_t *key,
                     const float *loglik_prop, float *cur_u, float *cur_log_target, float *cur_loglik, float *prop_u,
                     float *prop_log_prior, float *theta_prop, uint32_t *filter_key, float *sample_row, float *loglik_row,
                     float *target_row, int *n_accept, void *stream) {
    VSDE_CHECK_ARG(C >= 1 && R >= 1 && iteration >= 0, VSDE_E_BADARG, "vsde_pmmh_step: C %d, R %d >= 1 and iteration %d >= 0 expected",
                   C, R, iteration);
    VSDE_CHECK_ARG(P >= 1 && P <= kMcMaxP, VSDE_E_BADARG, "vsde_pmmh_step: P %d not supported (1..%d)", P, kMcMaxP);
    VSDE_CHECK_ARG((int64_t)C * R * P < ((int64_t)1 << 31), VSDE_E_BADARG, "vsde_pmmh_step: C R P = %lld elements: fewer than 2^31 expected",
                   (long long)C * R * P);
    VSDE_CHECK_ARG(scale_tril && key && cur_u && cur_log_target && cur_loglik && prop_u && prop_log_prior && theta_prop && filter_key &&
                   n_accept, VSDE_E_BADARG, "vsde_pmmh_step: NULL argument");
    VSDE_CHECK_ARG(iteration > 0 || !loglik_prop, VSDE_E_BADARG, "vsde_pmmh_step: iteration 0 has nothing to close (loglik_prop must be NULL)");
    VSDE_CHECK_ARG(step_size > 0 && step_size < INFINITY && prior_std > 0 && (prior_type == 0 || prior_type == 1), VSDE_E_BADARG,
                   "vsde_pmmh_step: bad step_size / prior");
    if (paths) {
        VSDE_CHECK_ARG(paths->N >= 1 && paths->K >= 1 && paths->S >= 1, VSDE_E_BADARG,
                       "vsde_pmmh_step_paths: N %d, K %d, S %d >= 1 expected", paths->N, paths->K, paths->S);
        VSDE_CHECK_ARG((int64_t)C * R * paths->N < ((int64_t)1 << 32), VSDE_E_BADARG,
                       "vsde_pmmh_step_paths: C R N = %lld paths (below 2^32 supported)", (long long)C * R * paths->N);
        VSDE_CHECK_ARG(paths->particles && paths->ancestors && paths->cur_anchor && paths->cur_noise && paths->cur_iter, VSDE_E_BADARG,
                       "vsde_pmmh_step_paths: NULL argument");
    }
    McParams p = {};
    for (int i = 0; i < P; ++i)
        for (int j = 0; j < P; ++j) {
            const float v = scale_tril[i * P + j];
            VSDE_CHECK_ARG(j <= i ? (v == v && fabsf(v) < INFINITY) : v == 0.f, VSDE_E_BADARG,
                           "vsde_pmmh_step: scale_tril[%d][%d] = %g: a finite lower-triangular matrix expected", i, j, (double)v);
            VSDE_CHECK_ARG(i != j || v > 0.f, VSDE_E_BADARG, "vsde_pmmh_step: scale_tril[%d][%d] = %g: a positive diagonal expected", i, j,
                           (double)v);
            p.L[i * P + j] = v;
        }
    p.C = C; p.R = R; p.iteration = iteration;
    p.pos_mask = em_mask(theta_positive_mask_host, P);
    p.prior_lognormal = prior_type; p.prior_mean = (float)prior_mean; p.prior_inv_std = (float)(1.0 / prior_std);
    p.prior_const = (float)(-log(prior_std) - 0.5 * log(2.0 * M_PI));
    p.step = (float)step_size; p.log_r = (float)log((double)R);
    p.key = key; p.loglik_prop = loglik_prop;
    p.cur_u = cur_u; p.cur_target = cur_log_target; p.cur_loglik = cur_loglik; p.prop_u = prop_u; p.prop_lp = prop_log_prior;
    p.theta_prop = theta_prop; p.filter_key = filter_key;
    p.sample_row = sample_row; p.loglik_row = loglik_row; p.target_row = target_row; p.n_accept = n_accept;
    const McPaths q = paths ? *paths : McPaths{};
    switch (P) {
#define VSDE_MC_CASE(n) case n: return paths ? pmmh_launch<n, true>(p, q, stream) : pmmh_launch<n, false>(p, q, stream);
        VSDE_MC_CASE(1) VSDE_MC_CASE(2) VSDE_MC_CASE(3) VSDE_MC_CASE(4) VSDE_MC_CASE(5) VSDE_MC_CASE(6) VSDE_MC_CASE(7) VSDE_MC_CASE(8)
        VSDE_MC_CASE(9) VSDE_MC_CASE(10) VSDE_MC_CASE(11) VSDE_MC_CASE(12) VSDE_MC_CASE(13) VSDE_MC_CASE(14) VSDE_MC_CASE(15) VSDE_MC_CASE(16)
#undef VSDE_MC_CASE
    }
    return VSDE_E_BADARG;
}

}  // namespace vsde

extern "C" int vsde_pmmh_step(int C, int P, int R, int iteration, const float *scale_tril, double step_size, int prior_type,
                              double prior_mean, double prior_std, const uint8_t *theta_positive_mask_host, const uint32_t *key,
                              const float *loglik_prop, float *cur_u, float *cur_log_target, float *cur_loglik, float *prop_u,
                              float *prop_log_prior, float *theta_prop, uint32_t *filter_key, float *sample_row, float *loglik_row,
                              float *target_row, int *n_accept, void *stream) {
    return vsde::pmmh_step(nullptr, C, P, R, iteration, scale_tril, step_size, prior_type, prior_mean, prior_std, theta_positive_mask_host,
                           key, loglik_prop, cur_u, cur_log_target, cur_loglik, prop_u, prop_log_prior, theta_prop, filter_key,
                           sample_row, loglik_row, target_row, n_accept, stream);
}

extern "C" int vsde_pmmh_step_paths(int C, int P, int R, int iteration, const float *scale_tril, double step_size, int prior_type,
                                    double prior_mean, double prior_std, const uint8_t *theta_positive_mask_host, const uint32_t *key,
                                    const float *loglik_prop, float *cur_u, float *cur_log_target, float *cur_loglik, float *prop_u,
                                    float *prop_log_prior, float *theta_prop, uint32_t *filter_key, float *sample_row,
                                    float *loglik_row, float *target_row, int *n_accept, int N, int K, int S, const float *particles,
                                    const int *ancestors, float *cur_anchor, uint32_t *cur_noise_path, int *cur_path_iteration,
                                    float *anchor_row, uint32_t *noise_row, int *iteration_row, void *stream) {
    const vsde::McPaths q = {N, K, S, particles, ancestors, cur_anchor, cur_noise_path, cur_path_iteration, anchor_row, noise_row,
                             iteration_row};
    return vsde::pmmh_step(&q, C, P, R, iteration, scale_tril, step_size, prior_type, prior_mean, prior_std, theta_positive_mask_host,
                           key, loglik_prop, cur_u, cur_log_target, cur_loglik, prop_u, prop_log_prior, theta_prop, filter_key,
                           sample_row, loglik_row, target_row, n_accept, stream);
}
