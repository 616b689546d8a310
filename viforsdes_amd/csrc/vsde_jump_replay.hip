// Replay of jump-process segments (gfx950): the latent paths of the jump-process particle smoother
// (viforsdes_amd/inference/jump_smoother.py) and of particle MCMC on the jump process (viforsdes_amd/inference/particle_mcmc.py,
// dynamics="jump"), read at output times that lie inside the segments.  The filter (vsde_jump_filter.hip) keeps the particles at
// the observations only; its noise is counter-based, philox4x32_10({e >> 1, k, b, 7}, key), so segment k of a path is recomputed
// exactly from its start state, its path slot b and theta.
//
// A thread per (segment k, record r), B records by K segments, k-major: idx = k B + r.  Neighbouring lanes replay the same segment
// of neighbouring records, whose event counts are alike; record-major would put a one-event segment and a thousand-event segment in
// the same wave.  256-thread workgroups, no LDS.  The int32 state x [S], the constants, the cumulative propensities and the float64
// clock live in registers; the chosen row of nu is read by compare-selects as in jf_kernel.
//
// The event is jf_kernel's word for word (same helpers, same expressions, same order): the clock restarts at exactly T_{k-1}
// (T_{-1} = 0) and the event counter at 0; fp32 propensities and cumulative sums; a NaN / infinite / negative a_j or an infinite a0
// -> status 2; tn = t + (double)(-logf(u1) / a0), a0 == 0 -> tn = inf; the segment ends as soon as T_k < tn; the reaction is the
// smallest j with u2 a0 < c_j, else the last j with a_j > 0; max_events events short of T_k -> status 1.
//
// Output times: path_times [Q] (float64, non-decreasing, 0 <= t_q <= T_{K-1}).  Segment k owns the t_q with T_{k-1} < t_q <= T_k
// (segment 0: 0 <= t_q <= T_0; a zero-length segment owns nothing): the outputs q_begin[k] .. q_begin[k+1] - 1, found by the host.
// Before the event at tn is applied every owned t_q < tn not yet written receives the current state: an output time receives the
// state after every event with time <= t_q (jump_kernel's rule).  A segment that ends with status 0 has written all its outputs by
// then; one that ends with status 1 or 2 leaves -1 in those it did not reach.
#include <hip/hip_runtime.h>

#include <cmath>

#include "vsde_sde_step.h"

namespace vsde {

constexpr int kJrMaxEvents = 1 << 23;   // vsde_jump.hip: kJumpMaxEvents
constexpr int kJrThreads = 256;
constexpr uint32_t kJrDeadPath = 0xFFFFFFFFu;

struct JrParams {
    int B, K, Q, P, N, D, max_events;   // B records; the filter form: B = M D, record r = m D + d
    const int32_t *x0;           // [M][S] (filter form) or [B][S]
    const float *theta;          // [M][P] or [B][P]: k (P = R), or the effective constants (k, K) (P = 2R)
    const double *times;         // [K] non-decreasing observation times
    const double *path_times;    // [Q] non-decreasing output times
    const int *q_begin;          // [K + 1]: segment k owns the outputs q_begin[k] .. q_begin[k + 1] - 1
    const uint32_t *keys;        // 2 words (filter form) or [B][2]
    const int32_t *particles;    // [M][K][N][S] (filter form)
    const int *ancestors;        // [M][K][N] (filter form)
    const int *last_slot;        // [M][D] (filter form; outside 0 .. N - 1: a dead filter)
    const int32_t *anchors;      // [B][K][S] (anchored form)
    const uint32_t *noise_path;  // [B][K] (anchored form; noise_path[K - 1] all ones: a dead record)
    int32_t *paths;              // [B][Q][S]
    int *lineage;                // [B][K] (filter form)
    int32_t *n_events, *status;  // [B][K]
    uint32_t orders[kCrnMaxR];   // reactant row of reaction j, 2 bits per species (crn_pack_orders)
    uint32_t nu[kCrnMaxR][2];    // net change of reaction j, one int8 per species: species 0..3, 4..7
    CrnNet net;
};

// Segment k of path b from the state x: jf_kernel's event loop, with the outputs q0 .. q1 - 1 of `out` ([Q][S]) written on the way.
// Returns the events fired; st: the status.
template <int S, int NR, bool KIN>
__device__ __forceinline__ int jr_segment(const JrParams &p, int (&x)[S], const float *th, int k, uint32_t b, uint32_t k0, uint32_t k1,
                                          int32_t *out, int q0, int q1, int &st) {
    const int R = p.net.R;
    const double t_k = p.times[k];
    double t = k ? p.times[k - 1] : 0.0;
    int ne = 0, q = q0;
    st = 1;                            // the status if the loop runs out of events
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
        // outputs before the event take the state before it
        while (q < q1 && p.path_times[q] < tn) {
#pragma unroll
            for (int i = 0; i < S; ++i) out[(int64_t)q * S + i] = x[i];
            ++q;
        }
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
    // status 0 has written every owned output (t_q <= T_k < tn); a stopped segment leaves -1 in those it did not reach
    for (; q < q1; ++q)
#pragma unroll
        for (int i = 0; i < S; ++i) out[(int64_t)q * S + i] = st == 0 ? x[i] : -1;
    return ne;
}

// ANCHORED = false: the smoother's form, a record is (filter m, draw d) and the thread traces its own slots through `ancestors`;
// true: the PMMH form, a record brings its theta, x0, key, anchors and noise paths.
template <int S, int NR, bool KIN, bool ANCHORED = false> __global__ void __launch_bounds__(kJrThreads) jr_kernel(JrParams p) {
    constexpr int P = KIN ? 2 * NR : NR;
    const int64_t g = (int64_t)blockIdx.x * kJrThreads + threadIdx.x;
    if (g >= (int64_t)p.B * p.K) return;
    const int k = (int)(g / p.B), r = (int)(g - (int64_t)k * p.B), Q = p.Q;
    // the ownership range, kept inside [0, Q] whatever the table holds
    const int q0 = min(max(p.q_begin[k], 0), Q), q1 = min(max(p.q_begin[k + 1], q0), Q);
    int32_t *out = p.paths + (int64_t)r * Q * S;
    const int64_t rk = (int64_t)r * p.K + k;
    int x[S];
    int row, slot = 0;
    uint32_t b, k0, k1;
    bool dead;
    if constexpr (ANCHORED) {
        const uint32_t *noise = p.noise_path + (int64_t)r * p.K;
        dead = noise[p.K - 1] == kJrDeadPath;
        row = r;
        b = noise[k]; k0 = p.keys[2 * (int64_t)r]; k1 = p.keys[2 * (int64_t)r + 1];
    } else {
        const int N = p.N;
        row = r / p.D;
        slot = p.last_slot[r];
        dead = slot < 0 || slot >= N;
        if (!dead) {
            // ancestors are slots of the same filter; the clamp keeps a corrupt entry inside its row
            const int *anc = p.ancestors + (int64_t)row * p.K * N;
            for (int kk = p.K - 1; kk > k; --kk) slot = min(max(anc[(int64_t)(kk - 1) * N + slot], 0), N - 1);
            if (k > 0) {
                const int prev = min(max(anc[(int64_t)(k - 1) * N + slot], 0), N - 1);
#pragma unroll
                for (int i = 0; i < S; ++i) x[i] = p.particles[(((int64_t)row * p.K + k - 1) * N + prev) * S + i];
            }
        }
        p.lineage[rk] = dead ? -1 : slot;
        b = (uint32_t)row * (uint32_t)N + (uint32_t)slot; k0 = p.keys[0]; k1 = p.keys[1];
    }
    if (dead) {
        // a dead filter or record has no path
        for (int q = q0; q < q1; ++q)
#pragma unroll
            for (int i = 0; i < S; ++i) out[(int64_t)q * S + i] = -1;
        p.n_events[rk] = 0;
        p.status[rk] = 0;
        return;
    }
    if (k == 0) {
#pragma unroll
        for (int i = 0; i < S; ++i) x[i] = p.x0[(int64_t)row * S + i];
    } else if constexpr (ANCHORED) {
#pragma unroll
        for (int i = 0; i < S; ++i) x[i] = p.anchors[((int64_t)r * p.K + k - 1) * S + i];
    }
    float th[P];
    if constexpr (KIN) crn_load_rates<NR>(th, p.theta, row, p.net.R, true);
    else em_load_theta<4, P>(th, p.theta, row, p.P, true);
    int st;
    const int ne = jr_segment<S, NR, KIN>(p, x, th, k, b, k0, k1, out, q0, q1, st);
    p.n_events[rk] = ne;
    p.status[rk] = st;
}

// One body for the four entry points.  Every check, the descriptors' included, comes before the first HIP call.  The filter form
// has B = M D records (N, D >= 1); the anchored form passes N = D = 0 and M = B.
static int jump_replay(const SdeRoute &rt, bool anchored, int M, int N, int D, int S, int P, int K, int Q, const int32_t *x0,
                       const float *theta, const double *obs_times, const double *path_times, const int *q_begin, const uint32_t *keys,
                       int max_events, const int32_t *particles, const int *ancestors, const int *last_slot, const int32_t *anchors,
                       const uint32_t *noise_path, int32_t *paths, int *lineage, int32_t *n_events, int32_t *status, void *stream) {
    JrParams p = {};
    const int rc = crn_route_net(rt, S, P, p.net);
    if (rc) return rc;
    VSDE_CHECK_ARG(M >= 1 && K >= 1, VSDE_E_BADARG, "jump replay: bad dims %s=%d K=%d", anchored ? "B" : "M", M, K);
    if (!anchored) {
        VSDE_CHECK_ARG(N >= 1 && D >= 1, VSDE_E_BADARG, "jump filter replay: %d particles, %d draws per filter (>= 1 supported)", N, D);
        VSDE_CHECK_ARG((int64_t)M * N < ((int64_t)1 << 32), VSDE_E_BADARG, "jump filter replay: M N = %lld paths (below 2^32 supported)",
                       (long long)M * N);
    }
    const int64_t B = anchored ? (int64_t)M : (int64_t)M * D;
    VSDE_CHECK_ARG(B * K < ((int64_t)1 << 31), VSDE_E_BADARG, "jump replay: %lld segments (below 2^31 supported)", (long long)(B * K));
    VSDE_CHECK_ARG(Q >= 1, VSDE_E_BADARG, "jump replay: %d output times (>= 1 supported)", Q);
    VSDE_CHECK_ARG(max_events >= 1 && max_events <= kJrMaxEvents, VSDE_E_BADARG, "jump replay: max_events %d outside 1..%d", max_events,
                   kJrMaxEvents);
    VSDE_CHECK_ARG(x0 && theta && obs_times && path_times && q_begin && keys && paths && n_events && status, VSDE_E_BADARG,
                   "jump replay: NULL argument");
    VSDE_CHECK_ARG(anchored ? (anchors && noise_path) : (particles && ancestors && last_slot && lineage), VSDE_E_BADARG,
                   "jump replay: NULL argument");
    p.B = (int)B; p.K = K; p.Q = Q; p.P = P; p.N = N; p.D = D; p.max_events = max_events;
    p.x0 = x0; p.theta = theta; p.times = obs_times; p.path_times = path_times; p.q_begin = q_begin; p.keys = keys;
    p.particles = particles; p.ancestors = ancestors; p.last_slot = last_slot; p.anchors = anchors; p.noise_path = noise_path;
    p.paths = paths; p.lineage = lineage; p.n_events = n_events; p.status = status;
    for (int j = 0; j < p.net.R; ++j) {
        p.orders[j] = crn_pack_orders(rt.net, j);
        for (int i = 0; i < S; ++i) p.nu[j][i >> 2] |= (uint32_t)(uint8_t)rt.net->change[j][i] << (8 * (i & 3));
    }
    const auto launch = [&](auto kern) {
        const int64_t threads = B * K;
        hipLaunchKernelGGL(kern, dim3((unsigned)((threads + kJrThreads - 1) / kJrThreads)), dim3(kJrThreads), 0, (hipStream_t)stream, p);
        VSDE_CHECK_HIP(hipGetLastError());
        return 0;
    };
    return crn_dispatch(S, p.net.R, [&](auto ns, auto nr) {
        constexpr int NS = decltype(ns)::value, NR = decltype(nr)::value;
        if (rt.descriptors == 2) return anchored ? launch(jr_kernel<NS, NR, true, true>) : launch(jr_kernel<NS, NR, true, false>);
        return anchored ? launch(jr_kernel<NS, NR, false, true>) : launch(jr_kernel<NS, NR, false, false>);
    });
}

}  // namespace vsde

using namespace vsde;

extern "C" int vsde_crn_jump_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int D, int Q,
                                           const int32_t *x0, const float *theta, const double *obs_times, const double *path_times,
                                           const int *q_begin, const uint32_t *key, int max_events, const int32_t *particles,
                                           const int *ancestors, const int *last_slot, int32_t *paths, int *lineage, int32_t *n_events,
                                           int32_t *status, void *stream) {
    return jump_replay(crn_route(net), false, M, N, D, S, P, K, Q, x0, theta, obs_times, path_times, q_begin, key, max_events, particles,
                       ancestors, last_slot, nullptr, nullptr, paths, lineage, n_events, status, stream);
}

extern "C" int vsde_crn_kinetic_jump_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                                   int K, int D, int Q, const int32_t *x0, const float *rates, const double *obs_times,
                                                   const double *path_times, const int *q_begin, const uint32_t *key, int max_events,
                                                   const int32_t *particles, const int *ancestors, const int *last_slot, int32_t *paths,
                                                   int *lineage, int32_t *n_events, int32_t *status, void *stream) {
    return jump_replay(crn_route(net, kin), false, M, N, D, S, P, K, Q, x0, rates, obs_times, path_times, q_begin, key, max_events,
                       particles, ancestors, last_slot, nullptr, nullptr, paths, lineage, n_events, status, stream);
}

extern "C" int vsde_crn_jump_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int Q, const int32_t *x0,
                                             const float *theta, const double *obs_times, const double *path_times, const int *q_begin,
                                             const int32_t *anchors, const uint32_t *noise_path, const uint32_t *keys, int max_events,
                                             int32_t *paths, int32_t *n_events, int32_t *status, void *stream) {
    return jump_replay(crn_route(net), true, B, 0, 0, S, P, K, Q, x0, theta, obs_times, path_times, q_begin, keys, max_events, nullptr,
                       nullptr, nullptr, anchors, noise_path, paths, nullptr, n_events, status, stream);
}

extern "C" int vsde_crn_kinetic_jump_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K,
                                                     int Q, const int32_t *x0, const float *rates, const double *obs_times,
                                                     const double *path_times, const int *q_begin, const int32_t *anchors,
                                                     const uint32_t *noise_path, const uint32_t *keys, int max_events, int32_t *paths,
                                                     int32_t *n_events, int32_t *status, void *stream) {
    return jump_replay(crn_route(net, kin), true, B, 0, 0, S, P, K, Q, x0, rates, obs_times, path_times, q_begin, keys, max_events,
                       nullptr, nullptr, nullptr, anchors, noise_path, paths, nullptr, n_events, status, stream);
}
