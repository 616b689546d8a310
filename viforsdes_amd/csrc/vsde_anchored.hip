// Replay of carried path records (gfx950): the paths of particle MCMC (viforsdes_amd/inference/particle_mcmc.py is the
// specification).  A translation unit of its own, next to vsde_filter.hip, so that the two compile side by side; the step code is
// the shared vsde_filter_step.h, the kernel (ar_kernel) and its host body are in vsde_filter_kernels.h.
#include "vsde_filter_kernels.h"

using namespace vsde;

// Replay of carried path records (particle MCMC with paths): every record brings its own start state, theta, key, anchors and
// noise paths
extern "C" int vsde_anchored_replay(int kind, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta,
                                    const int *obs_rows, const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                    double time_step, const uint8_t *positive_mask_host, float *paths, void *stream) {
    return anchored_replay(SdeRoute{kind}, false, B, S, P, K, O, T, x0, theta, obs_rows, nullptr, nullptr, 1.0, anchors, noise_path,
                           keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_crn_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int O, int T, const float *x0,
                                        const float *theta, const int *obs_rows, const float *anchors, const uint32_t *noise_path,
                                        const uint32_t *keys, double time_step, const uint8_t *positive_mask_host, float *paths,
                                        void *stream) {
    return anchored_replay(crn_route(net), false, B, S, P, K, O, T, x0, theta, obs_rows, nullptr, nullptr, 1.0, anchors, noise_path,
                           keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_crn_kinetic_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K,
                                                int O, int T, const float *x0, const float *rates, const int *obs_rows,
                                                const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                                double time_step, const uint8_t *positive_mask_host, float *paths, void *stream) {
    return anchored_replay(crn_route(net, kin), false, B, S, P, K, O, T, x0, rates, obs_rows, nullptr, nullptr, 1.0, anchors,
                           noise_path, keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_guided_anchored_replay(int kind, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta,
                                           const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                           const float *anchors, const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                           const uint8_t *positive_mask_host, float *paths, void *stream) {
    return anchored_replay(SdeRoute{kind}, true, B, S, P, K, O, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, anchors,
                           noise_path, keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_crn_guided_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int O, int T, const float *x0,
                                               const float *theta, const int *obs_rows, const float *obs_values,
                                               const float *obs_matrix, double variance, const float *anchors,
                                               const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                               const uint8_t *positive_mask_host, float *paths, void *stream) {
    return anchored_replay(crn_route(net), true, B, S, P, K, O, T, x0, theta, obs_rows, obs_values, obs_matrix, variance, anchors,
                           noise_path, keys, time_step, positive_mask_host, paths, stream);
}

extern "C" int vsde_crn_kinetic_guided_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P,
                                                       int K, int O, int T, const float *x0, const float *rates, const int *obs_rows,
                                                       const float *obs_values, const float *obs_matrix, double variance,
                                                       const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                                       double time_step, const uint8_t *positive_mask_host, float *paths,
                                                       void *stream) {
    return anchored_replay(crn_route(net, kin), true, B, S, P, K, O, T, x0, rates, obs_rows, obs_values, obs_matrix, variance, anchors,
                           noise_path, keys, time_step, positive_mask_host, paths, stream);
}
