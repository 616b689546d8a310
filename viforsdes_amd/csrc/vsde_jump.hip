// Exact simulation of the Markov jump process of a reaction network (Gillespie's direct method) on integer copy numbers: the
// process whose diffusion approximation the kind-4 routes run.  viforsdes_amd/core/jump_process.py is the specification.
//
// A thread per trajectory, 64-thread workgroups.  The descriptor travels by value in the argument block; x [S] (int32), the
// constants, the cumulative propensities and the float64 clock live in registers from the first event to the last: memory traffic
// is x0, theta, the key and the output times in, the outputs (and the optional event log) out.
//
// Event e (0-based) of path b:  a_j = crn_jump_propensity, c_j = a_0 + .. + a_j in reaction order (fp32), a0 = c_{R-1}.
//   a NaN, infinite or negative a_j (or an infinite a0)       -> the path stops with status 2
//   a0 == 0                                                   -> absorbed: every remaining output is the current state, status 0
//   tau = -logf(u1) / a0 (fp32),  t += (double)tau            -> outputs with T_k < t take the state before the event
//   reaction: the smallest j with u2 a0 < c_j, else the last j with a_j > 0;  x += nu_j
// with (u1, u2) = uniforms 2 (e & 1), 2 (e & 1) + 1 of philox4x32_10({e >> 1, 0, b, 7}, key).  The only loop over events counts
// e up to max_events and the only loop over outputs counts k up to K, whatever the constants are: a path still short of its last
// output time after max_events events stops with status 1 and -1 in the outputs it did not reach.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vsde_sde_step.h"

namespace vsde {

constexpr int kJumpMaxEvents = 1 << 23;   // x0 <= 2^30 and |nu| <= 127: 2^30 + 127 * 2^23 < 2^31, the int32 state cannot overflow

struct JumpParams {
    int B, K, E, P, max_events;
    const int32_t *x0;       // [B][S]
    const float *theta;      // [B][P]: k (P = R), or the effective constants (k, K) (P = 2R)
    const double *times;     // [K] non-decreasing output times
    const uint32_t *key;     // 2 words
    int32_t *states;         // [B][K][S]
    int32_t *n_events, *status;   // [B]
    double *ev_time;         // [B][E] or NULL
    int32_t *ev_reaction;    // [B][E] or NULL
    uint32_t orders[kCrnMaxR];   // reactant row of reaction j, 2 bits per species (crn_pack_orders)
    uint32_t nu[kCrnMaxR][2];    // net change of reaction j, one int8 per species: species 0..3, 4..7
    CrnNet net;                  // R and the rate-law tables
};

template <int S, int NR, bool KIN> __global__ void __launch_bounds__(64) jump_kernel(JumpParams p) {
    constexpr int P = KIN ? 2 * NR : NR;
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    const int R = p.net.R;
    const uint32_t k0 = p.key[0], k1 = p.key[1];
    int x[S];
    float th[P];
#pragma unroll
    for (int i = 0; i < S; ++i) x[i] = p.x0[(int64_t)b * S + i];
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, b, R, true);
    else em_load_theta<4, P>(th, p.theta, b, p.P, true);
    int32_t *out = p.states + (int64_t)b * p.K * S;
    double t = 0.0;
    int k = 0, ne = 0, st = 0;
    uint4 w = make_uint4(0u, 0u, 0u, 0u);
    for (int e = 0; e < p.max_events; ++e) {
        float xf[S], c[NR];
#pragma unroll
        for (int i = 0; i < S; ++i) xf[i] = (float)x[i];
        float acc = 0.f;
        bool bad = false;
        int jlast = 0;                     // the last reaction with a_j > 0
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (j < R) {
                const float a = crn_jump_propensity<S, NR, KIN>(p.net, p.orders[j], j, x, xf, th);
                bad = bad || !(a >= 0.f) || a == INFINITY;
                if (a > 0.f) jlast = j;
                acc += a;
            }
            c[j] = acc;
        }
        const float a0 = acc;
        if (bad || a0 == INFINITY) { st = 2; break; }
        if ((e & 1) == 0) w = philox4x32_10(make_uint4((uint32_t)e >> 1, 0u, (uint32_t)b, 7u), k0, k1);
        const float u1 = philox_uniform((e & 1) ? w.z : w.x), u2 = philox_uniform((e & 1) ? w.w : w.y);
        const double tn = a0 == 0.f ? (double)INFINITY : t + (double)(-logf(u1) / a0);
        while (k < p.K && p.times[k] < tn) {
#pragma unroll
            for (int i = 0; i < S; ++i) out[(int64_t)k * S + i] = x[i];
            ++k;
        }
        if (k >= p.K) break;
        const float thr = u2 * a0;
        int js = -1;
#pragma unroll
        for (int j = NR - 1; j >= 0; --j)
            if (j < R && thr < c[j]) js = j;
        if (js < 0) js = jlast;
        // the chosen row (8 int8 in two words) by compare-selects over the uniform table: indexing the table by the lane's js
        // would go to scratch
        uint32_t lo = 0u, hi = 0u;
#pragma unroll
        for (int j = 0; j < NR; ++j)
            if (j == js) {
                lo = p.nu[j][0];
                if constexpr (S > 4) hi = p.nu[j][1];
            }
#pragma unroll
        for (int i = 0; i < S; ++i) x[i] += (int)(int8_t)((i < 4 ? lo : hi) >> (8 * (i & 3)));
        t = tn;
        if (ne < p.E) {
            p.ev_time[(int64_t)b * p.E + ne] = t;
            p.ev_reaction[(int64_t)b * p.E + ne] = js;
        }
        ++ne;
    }
    if (k < p.K && st == 0) st = 1;
    for (; k < p.K; ++k) {
#pragma unroll
        for (int i = 0; i < S; ++i) out[(int64_t)k * S + i] = -1;
    }
    for (int e = ne; e < p.E; ++e) {
        p.ev_time[(int64_t)b * p.E + e] = (double)NAN;
        p.ev_reaction[(int64_t)b * p.E + e] = -1;
    }
    p.n_events[b] = ne;
    p.status[b] = st;
}

// every check, the descriptors' included, comes before the first HIP call
static int jump_process(const SdeRoute &rt, int B, int S, int P, int K, int E, const int32_t *x0, const float *theta,
                        const double *out_times, const uint32_t *key, int max_events, int32_t *states, int32_t *n_events,
                        int32_t *status, double *event_times, int32_t *event_reactions, void *stream) {
    JumpParams p = {};
    const int rc = crn_route_net(rt, S, P, p.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(B >= 1 && K >= 1 && E >= 0, VSDE_E_BADARG, "bad jump-process dims B=%d K=%d E=%d", B, K, E);
    VSDE_CHECK_ARG(max_events >= 1 && max_events <= kJumpMaxEvents, VSDE_E_BADARG, "jump process: max_events %d outside 1..%d",
                   max_events, kJumpMaxEvents);
    VSDE_CHECK_ARG(x0 && theta && out_times && key && states && n_events && status, VSDE_E_BADARG, "jump process: NULL argument");
    VSDE_CHECK_ARG(E == 0 || (event_times && event_reactions), VSDE_E_BADARG, "jump process: E=%d events to log but a NULL log pointer",
                   E);
    p.B = B; p.K = K; p.E = E; p.P = P; p.max_events = max_events;
    for (int j = 0; j < p.net.R; ++j) {
        p.orders[j] = crn_pack_orders(rt.net, j);
        for (int i = 0; i < S; ++i) p.nu[j][i >> 2] |= (uint32_t)(uint8_t)rt.net->change[j][i] << (8 * (i & 3));
    }
    p.x0 = x0; p.theta = theta; p.times = out_times; p.key = key;
    p.states = states; p.n_events = n_events; p.status = status; p.ev_time = event_times; p.ev_reaction = event_reactions;
    const dim3 grid((unsigned)((B + 63) / 64)), block(64);
    return crn_dispatch(S, p.net.R, [&](auto ns, auto nr) {
        constexpr int NS = decltype(ns)::value, NR = decltype(nr)::value;
        if (rt.descriptors == 2) hipLaunchKernelGGL((jump_kernel<NS, NR, true>), grid, block, 0, (hipStream_t)stream, p);
        else hipLaunchKernelGGL((jump_kernel<NS, NR, false>), grid, block, 0, (hipStream_t)stream, p);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    });
}

}  // namespace vsde

using namespace vsde;

extern "C" int vsde_crn_jump_process(const vsde_crn_network *net, int B, int S, int P, int K, int E, const int32_t *x0,
                                     const float *theta, const double *out_times, const uint32_t *key, int max_events,
                                     int32_t *states, int32_t *n_events, int32_t *status, double *event_times,
                                     int32_t *event_reactions, void *stream) {
    return jump_process(crn_route(net), B, S, P, K, E, x0, theta, out_times, key, max_events, states, n_events, status, event_times,
                        event_reactions, stream);
}

extern "C" int vsde_crn_kinetic_jump_process(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K,
                                             int E, const int32_t *x0, const float *rates, const double *out_times,
                                             const uint32_t *key, int max_events, int32_t *states, int32_t *n_events,
                                             int32_t *status, double *event_times, int32_t *event_reactions, void *stream) {
    return jump_process(crn_route(net, kin), B, S, P, K, E, x0, rates, out_times, key, max_events, states, n_events, status,
                        event_times, event_reactions, stream);
}
