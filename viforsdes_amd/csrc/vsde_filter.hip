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
// The particle smoother's replay kernel (rp_kernel) runs single segments of a filter again from the stored particles and
// ancestors, through the same pf_propagate / pf_propagate_guided with a store hook.  That step code and the argument block live in
// vsde_filter_step.h, the kernel templates and their host bodies in vsde_filter_kernels.h: the replay of carried path records
// (particle MCMC with paths: vsde_anchored.hip) and the residual-bridge forms of all three kernels (vsde_residual.hip) share them
// from translation units of their own.  This file holds the entry points of the filter and of the genealogy replay.
#include "vsde_filter_kernels.h"

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
