// Residual-bridge proposal of the guided particle filter (gfx950; proposal = "residual_bridge",
// viforsdes_amd/inference/particle_filter.py is the specification): the RES instantiations of the filter kernel, of the replay of
// its genealogy and of the replay of carried path records, behind entry points that mirror the nine guided ones.  A translation
// unit of its own: vsde_filter.hip and vsde_anchored.hip compile what they always did, and the three build side by side.
// The step is the bridge step with one quantity replaced: the predicted state at the observation's row, x + n dt f(x), becomes
// eta_end + (x - eta) + n dt (f(x) - f(eta)), where eta is the noise-free Euler path from the segment's start state (carried in
// registers next to x and advanced with every step) and eta_end its end at that row (from a drift-only pass at segment entry).
// Both replays restart a segment from its stored start state, so they form the same eta and repeat the filter's states bit for bit.
#include "vsde_filter_kernels.h"

using namespace vsde;

extern "C" int vsde_residual_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                                             const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                             const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                             float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                             float *filtered_std, float *particles, int *ancestors, float *log_weights, void *stream) {
    return particle_filter<true>(SdeRoute{kind}, true, nullptr, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, variance,
                                 key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                                 particles, ancestors, log_weights, stream);
}

extern "C" int vsde_crn_residual_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                                 const float *theta, const int *obs_rows, const float *obs_values,
                                                 const float *obs_matrix, double variance, const uint32_t *key, double time_step,
                                                 const uint8_t *positive_mask_host, float *log_likelihood, float *increments,
                                                 float *ess, float *filtered_mean, float *filtered_std, float *particles,
                                                 int *ancestors, float *log_weights, void *stream) {
    return particle_filter<true>(crn_route(net), true, nullptr, M, N, S, P, K, O, x0, theta, obs_rows, obs_values, obs_matrix, variance,
                                 key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean, filtered_std,
                                 particles, ancestors, log_weights, stream);
}

extern "C" int vsde_crn_kinetic_residual_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                         int P, int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                                         const float *obs_values, const float *obs_matrix, double variance,
                                                         const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                                         float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                                         float *filtered_std, float *particles, int *ancestors, float *log_weights,
                                                         void *stream) {
    return particle_filter<true>(crn_route(net, kin), true, nullptr, M, N, S, P, K, O, x0, rates, obs_rows, obs_values, obs_matrix,
                                 variance, key, time_step, positive_mask_host, log_likelihood, increments, ess, filtered_mean,
                                 filtered_std, particles, ancestors, log_weights, stream);
}

extern "C" int vsde_residual_filter_replay(int kind, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0,
                                           const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                           double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                           const float *particles, const int *ancestors, const int *last_slot, float *paths,
                                           int *lineage, void *stream) {
    return filter_replay<true>(SdeRoute{kind}, true, M, N, S, P, K, O, D, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, key,
                               time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_crn_residual_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, int D, int T,
                                               const float *x0, const float *theta, const int *obs_rows, const float *obs_values,
                                               const float *obs_matrix, double variance, const uint32_t *key, double time_step,
                                               const uint8_t *positive_mask_host, const float *particles, const int *ancestors,
                                               const int *last_slot, float *paths, int *lineage, void *stream) {
    return filter_replay<true>(crn_route(net), true, M, N, S, P, K, O, D, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, key,
                               time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_crn_kinetic_residual_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S,
                                                       int P, int K, int O, int D, int T, const float *x0, const float *rates,
                                                       const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                                       double variance, const uint32_t *key, double time_step,
                                                       const uint8_t *positive_mask_host, const float *particles, const int *ancestors,
                                                       const int *last_slot, float *paths, int *lineage, void *stream) {
    return filter_replay<true>(crn_route(net, kin), true, M, N, S, P, K, O, D, T, x0, rates, obs_rows, obs_values, obs_matrix, variance,
                               key, time_step, positive_mask_host, particles, ancestors, last_slot, paths, lineage, stream);
}

extern "C" int vsde_residual_anchored_replay(int kind, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta,
                                             const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                             const float *anchors, const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                             const uint8_t *positive_mask_host, float *paths, void *stream) {
    return anchored_replay<true>(SdeRoute{kind}, true, B, S, P, K, O, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, anchors,
                                 noise_path, keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_crn_residual_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int O, int T, const float *x0,
                                                 const float *theta, const int *obs_rows, const float *obs_values,
                                                 const float *obs_matrix, double variance, const float *anchors,
                                                 const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                                 const uint8_t *positive_mask_host, float *paths, void *stream) {
    return anchored_replay<true>(crn_route(net), true, B, S, P, K, O, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, anchors,
                                 noise_path, keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_crn_kinetic_residual_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P,
                                                         int K, int O, int T, const float *x0, const float *rates, const int *obs_rows,
                                                         const float *obs_values, const float *obs_matrix, double variance,
                                                         const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                                         double time_step, const uint8_t *positive_mask_host, float *paths,
                                                         void *stream) {
    return anchored_replay<true>(crn_route(net, kin), true, B, S, P, K, O, T, x0, rates, obs_rows, obs_values, obs_matrix, variance,
                                 anchors, noise_path, keys, time_step, positive_mask_host, paths, stream);
}
