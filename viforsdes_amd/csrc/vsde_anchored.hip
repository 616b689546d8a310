// Replay of carried path records (gfx950): the paths of particle MCMC (viforsdes_amd/inference/particle_mcmc.py is the
// specification).  A translation unit of its own, next to vsde_filter.hip, so that the two compile side by side; the step code is
// the shared vsde_filter_step.h.
#include "vsde_filter_step.h"

namespace vsde {

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

template <int KIND, int NS = EmDims<KIND>::S, int NR = EmDims<KIND>::P, bool KIN = false, int NO = 0>
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
        pf_propagate_guided<KIND, NS, NR, KIN, NO>(p, x, th, t0, t1, nb, k0, k1, p.obs_values + (int64_t)k * p.O, lr, st);
    } else {
        pf_propagate<KIND, NS, NR, KIN, P>(p, x, th, t0, t1, nb, k0, k1, b, st);
    }
}

// One body for the vsde_*anchored_replay entry points: any route, plain or guided.  Every check comes before the first HIP call.
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

}  // namespace vsde

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
