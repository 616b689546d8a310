// Monte-Carlo ELBO accumulation over sample paths (gfx950): SDE transition log-density,
// variational path entropy (generative log-density) and softplus log-Jacobian, forward and
// analytic adjoint.  Replaces the two MultivariateNormal(scale_tril=...).log_prob calls over
// B*T tiny matrices plus ~10 elementwise torch kernels of the reference
// (src/variational_sde/inference/evidence_lower_bound.py:42-50,77-83; inference/types.py:23-24;
// inference/state_space.py:35-38).  HBM-bound streaming kernels: every tensor is read once.
#include "vsde_sde_coef.h"

namespace vsde {

constexpr float kLog2Pi = 1.8378770664093453f;
constexpr int kElboBwdMaxPaths = 65535;   // elbo_path_terms_bwd_kernel: one gridDim.y row per path

struct ElboParams {
    int B, T;
    const float *z, *x, *means, *chol, *drift, *diffusion;
    uint32_t pos_mask;
    float dt, sqdt;
    // forward outputs
    float *sde_lp, *gen_lp, *jac;
    // backward
    const float *g_sde, *g_gen, *g_jac;
    float *g_z, *g_x, *g_means, *g_chol, *g_drift, *g_diffusion;
};

// w = (A*s)^-1 (y - (m0 + d*dt)); returns log N(y; m0 + d dt, (A s)(A s)^T)
template <int S>
__device__ __forceinline__ float tri_logpdf(const float *__restrict__ y, const float *__restrict__ m0,
                                            const float *__restrict__ d, const float *__restrict__ A, float dt, float s,
                                            float (&w)[S]) {
    float quad = 0.f, logdet = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        float acc = y[i] - (m0[i] + d[i] * dt);
#pragma unroll
        for (int j = 0; j < i; ++j) acc -= (A[i * S + j] * s) * w[j];
        float dii = A[i * S + i] * s;
        w[i] = acc / dii;
        quad += w[i] * w[i];
        logdet += __logf(dii);
    }
    return -0.5f * ((float)S * kLog2Pi + quad) - logdet;
}

__device__ __forceinline__ float log_sigmoid(float v) { return fminf(v, 0.f) - log1pf(__expf(-fabsf(v))); }

template <int S>
__global__ void __launch_bounds__(256) elbo_path_terms_kernel(ElboParams p) {
    const int b = blockIdx.x;
    float s_acc = 0.f, g_acc = 0.f, j_acc = 0.f;
    for (int t = threadIdx.x; t < p.T; t += blockDim.x) {
        const int64_t o1 = ((int64_t)b * (p.T + 1) + t) * S, o2 = ((int64_t)b * p.T + t) * S;
        float w[S];
        s_acc += tri_logpdf<S>(p.x + o1 + S, p.x + o1, p.drift + o2, p.diffusion + o2 * S, p.dt, p.sqdt, w);
        g_acc += tri_logpdf<S>(p.z + o1 + S, p.z + o1, p.means + o2, p.chol + o2 * S, p.dt, p.sqdt, w);
#pragma unroll
        for (int i = 0; i < S; ++i)
            if ((p.pos_mask >> i) & 1u) j_acc += log_sigmoid(p.z[o1 + S + i]);
    }
    __shared__ float red[3][4];
    s_acc = wave_sum(s_acc); g_acc = wave_sum(g_acc); j_acc = wave_sum(j_acc);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) { red[0][wave] = s_acc; red[1][wave] = g_acc; red[2][wave] = j_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = blockDim.x >> 6;
        float a = 0.f, c = 0.f, d = 0.f;
        for (int i = 0; i < nw; ++i) { a += red[0][i]; c += red[1][i]; d += red[2][i]; }
        p.sde_lp[b] = a; p.gen_lp[b] = c; p.jac[b] = d;
    }
}

// v = (A s)^-T w
template <int S>
__device__ __forceinline__ void tri_solve_t(const float *__restrict__ A, float s, const float (&w)[S], float (&v)[S]) {
#pragma unroll
    for (int i = S - 1; i >= 0; --i) {
        float acc = w[i];
#pragma unroll
        for (int j = i + 1; j < S; ++j) acc -= (A[j * S + i] * s) * v[j];
        v[i] = acc / (A[i * S + i] * s);
    }
}

// One thread per (b, tau), tau in [0, T]: the "current" role of step tau (local gradients and the
// +v term of g_z/g_x[tau]) and the "next" role of step tau-1 (the -v term), so nothing races.
template <int S>
__global__ void __launch_bounds__(256) elbo_path_terms_bwd_kernel(ElboParams p) {
    const int b = blockIdx.y, tau = blockIdx.x * blockDim.x + threadIdx.x;
    if (tau > p.T) return;
    const float gs = p.g_sde[b], gg = p.g_gen[b], gj = p.g_jac[b];
    float gz[S], gx[S];
#pragma unroll
    for (int i = 0; i < S; ++i) { gz[i] = 0.f; gx[i] = 0.f; }
    float w[S], v[S];
    if (tau < p.T) {
        const int64_t o1 = ((int64_t)b * (p.T + 1) + tau) * S, o2 = ((int64_t)b * p.T + tau) * S;
        const float *G = p.diffusion + o2 * S, *Lc = p.chol + o2 * S;
        (void)tri_logpdf<S>(p.x + o1 + S, p.x + o1, p.drift + o2, G, p.dt, p.sqdt, w);
        tri_solve_t<S>(G, p.sqdt, w, v);
#pragma unroll
        for (int i = 0; i < S; ++i) {
            gx[i] += gs * v[i];
            p.g_drift[o2 + i] = gs * v[i] * p.dt;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                float val = j <= i ? gs * p.sqdt * v[i] * w[j] : 0.f;
                if (i == j) val -= gs / G[i * S + i];
                p.g_diffusion[o2 * S + i * S + j] = val;
            }
        }
        (void)tri_logpdf<S>(p.z + o1 + S, p.z + o1, p.means + o2, Lc, p.dt, p.sqdt, w);
        tri_solve_t<S>(Lc, p.sqdt, w, v);
#pragma unroll
        for (int i = 0; i < S; ++i) {
            gz[i] += gg * v[i];
            p.g_means[o2 + i] = gg * v[i] * p.dt;
#pragma unroll
            for (int j = 0; j < S; ++j) {
                float val = j <= i ? gg * p.sqdt * v[i] * w[j] : 0.f;
                if (i == j) val -= gg / Lc[i * S + i];
                p.g_chol[o2 * S + i * S + j] = val;
            }
        }
    }
    if (tau > 0) {
        const int64_t o1 = ((int64_t)b * (p.T + 1) + tau - 1) * S, o2 = ((int64_t)b * p.T + tau - 1) * S;
        (void)tri_logpdf<S>(p.x + o1 + S, p.x + o1, p.drift + o2, p.diffusion + o2 * S, p.dt, p.sqdt, w);
        tri_solve_t<S>(p.diffusion + o2 * S, p.sqdt, w, v);
#pragma unroll
        for (int i = 0; i < S; ++i) gx[i] -= gs * v[i];
        (void)tri_logpdf<S>(p.z + o1 + S, p.z + o1, p.means + o2, p.chol + o2 * S, p.dt, p.sqdt, w);
        tri_solve_t<S>(p.chol + o2 * S, p.sqdt, w, v);
#pragma unroll
        for (int i = 0; i < S; ++i) {
            gz[i] -= gg * v[i];
            if ((p.pos_mask >> i) & 1u) gz[i] += gj * fast_rcp(1.0f + __expf(p.z[o1 + S + i]));  // d logsigmoid = sigmoid(-z)
        }
    }
    const int64_t o = ((int64_t)b * (p.T + 1) + tau) * S;
#pragma unroll
    for (int i = 0; i < S; ++i) { p.g_z[o + i] = gz[i]; p.g_x[o + i] = gx[i]; }
}

template <int S>
static int launch_elbo(const ElboParams &p, bool bwd, hipStream_t s) {
    if (!bwd) hipLaunchKernelGGL((elbo_path_terms_kernel<S>), dim3(p.B), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((elbo_path_terms_bwd_kernel<S>), dim3((p.T + 1 + 255) / 256, p.B), dim3(256), 0, s, p);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

static int dispatch_elbo(int S, const ElboParams &p, bool bwd, hipStream_t s) {
    switch (S) {
        case 1: return launch_elbo<1>(p, bwd, s);
        case 2: return launch_elbo<2>(p, bwd, s);
        case 3: return launch_elbo<3>(p, bwd, s);
        case 4: return launch_elbo<4>(p, bwd, s);
        case 5: return launch_elbo<5>(p, bwd, s);
        case 6: return launch_elbo<6>(p, bwd, s);
        case 7: return launch_elbo<7>(p, bwd, s);
        case 8: return launch_elbo<8>(p, bwd, s);
        case 9: return launch_elbo<9>(p, bwd, s);
        case 10: return launch_elbo<10>(p, bwd, s);
        case 11: return launch_elbo<11>(p, bwd, s);
        case 12: return launch_elbo<12>(p, bwd, s);
        case 13: return launch_elbo<13>(p, bwd, s);
        case 14: return launch_elbo<14>(p, bwd, s);
        case 15: return launch_elbo<15>(p, bwd, s);
        case 16: return launch_elbo<16>(p, bwd, s);
        default:
            set_error("state_dim %d not supported by the ELBO kernels (1..16)", S);
            return VSDE_E_STATE;
    }
}

static uint32_t mask_bits(const uint8_t *m, int S) {
    uint32_t r = 0;
    if (m) for (int i = 0; i < S; ++i) if (m[i]) r |= 1u << i;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------
// The [B]-sized tail of the ELBO (inference/evidence_lower_bound.py:52-83 of the reference): Gaussian (or, CNT, count) observation log-density
// at the observed grid points (core/observations.py:57-74), iid Normal / LogNormal prior (core/priors.py:46-60), mean-field
// (Log)Normal posterior log q(theta) (models/sde_parameter_posterior.py:44-66), and the batch means
//   out = [ mean_b(obs + sde - gen + jac + prior - post), mean obs, mean sde, mean gen, mean prior, mean post ].
// ~50 tiny torch kernels forward and ~100 in autograd's backward become one single-workgroup kernel each (B is a few hundred to
// a few thousand; the work is microseconds, the launches were not).  Sums over b in a fixed tree: deterministic.
struct TailParams {
    int B, K, S, O, P;
    const float *x_obs;        // [B][K][S] states at the observed grid points
    const float *obs_values;   // [K][O]
    const float *obs_matrix;   // [O][S] or nullptr (identity, O == S)
    float inv_var, log_norm;   // 1 / variance, -0.5 log(2 pi variance)
    const float *theta;        // [B][P]
    int prior_lognormal; float prior_mean, prior_inv_std, prior_const;   // const = -log(std) - 0.5 log(2 pi)
    const float *post_mean, *post_log_std;   // [P]
    uint32_t theta_pos;
    const float *sde_lp, *gen_lp, *jac;      // [B]
    float *out;                // [6]
    const float *g_out;        // [6]
    float *g_x_obs, *g_theta, *g_post_mean, *g_post_log_std, *g_sde, *g_gen, *g_jac;
};

constexpr int kTailMaxDim = 16;   // S, O, P <= 16 (P <= 32 for the mask; the per-thread arrays set the smaller bound)

template <int N> __device__ __forceinline__ void tail_block_sum(float (*red)[N], float (&v)[N], int tid) {
#pragma unroll
    for (int i = 0; i < N; ++i) red[tid][i] = v[i];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int i = 0; i < N; ++i) red[tid][i] += red[tid + w][i];
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = red[0][i];
    __syncthreads();
}

// the states of path b at its observed grid points, read from x_obs [B][K][S]
struct XObsRows {
    const TailParams &p;
    int b;
    __device__ float operator()(int k, int i) const { return p.x_obs[((int64_t)b * p.K + k) * p.S + i]; }
};

// observation term of path b, its state at observation k read as x(k, i); when GX, also d obs_lp / d x_obs scaled by w
// CNT: the count term c (vsde_sde_coef.h: count_term) in place of the Gaussian one
template <bool GX, bool CNT, class X>
__device__ __forceinline__ float tail_obs(const TailParams &p, const CountLik &c, int b, float w, const X &x) {
    float lp = 0.f;
    for (int k = 0; k < p.K; ++k) {
        float *gx = GX ? p.g_x_obs + ((int64_t)b * p.K + k) * p.S : nullptr;
        if (GX) for (int i = 0; i < p.S; ++i) gx[i] = 0.f;
        if constexpr (CNT) lp += c.row_const[k];
        for (int o = 0; o < p.O; ++o) {
            float pred;
            if (p.obs_matrix) {
                pred = 0.f;
                for (int i = 0; i < p.S; ++i) pred += p.obs_matrix[o * p.S + i] * x(k, i);
            } else {
                pred = x(k, o);
            }
            [[maybe_unused]] float dterm = 0.f;   // count term: d term / d pred
            const float r = p.obs_values[k * p.O + o] - pred;
            if constexpr (CNT) lp += count_term<GX>(c, p.obs_values[k * p.O + o], pred, dterm);
            else lp += -0.5f * r * r * p.inv_var + p.log_norm;
            if (GX) {
                const float gr = CNT ? w * dterm : w * r * p.inv_var;   // d lp / d pred
                if (p.obs_matrix) for (int i = 0; i < p.S; ++i) gx[i] += gr * p.obs_matrix[o * p.S + i];
                else gx[o] += gr;
            }
        }
    }
    return lp;
}

// per-sample tail of path b: observation log-density, log prior and log posterior of theta_b (the ELBO tail and the importance
// log-weight kernel evaluate exactly this)
struct TailTerms { float obs, prior, post; };

template <bool CNT, class X>
__device__ __forceinline__ TailTerms tail_terms(const TailParams &p, const CountLik &c, int b, const X &x) {
    TailTerms r;
    r.obs = tail_obs<false, CNT>(p, c, b, 0.f, x);
    float prior = 0.f, post = 0.f;
    for (int i = 0; i < p.P; ++i) {
        const float th = p.theta[(int64_t)b * p.P + i];
        const bool pos = (p.theta_pos >> i) & 1u;
        const float lg = (pos || p.prior_lognormal) ? logf(th) : 0.f;
        const float zp = ((p.prior_lognormal ? lg : th) - p.prior_mean) * p.prior_inv_std;
        prior += -0.5f * zp * zp + p.prior_const - (p.prior_lognormal ? lg : 0.f);
        const float ls = p.post_log_std[i];
        const float zq = ((pos ? lg : th) - p.post_mean[i]) * expf(-ls);
        post += -0.5f * zq * zq - ls - 0.5f * kLog2Pi - (pos ? lg : 0.f);
    }
    r.prior = prior; r.post = post;
    return r;
}

template <bool CNT> __global__ void __launch_bounds__(256) elbo_tail_fwd_kernel(TailParams p, CountLik c) {
    __shared__ float red[256][6];
    const int tid = threadIdx.x;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b = tid; b < p.B; b += 256) {
        const TailTerms tt = tail_terms<CNT>(p, c, b, XObsRows{p, b});
        const float obs = tt.obs, prior = tt.prior, post = tt.post;
        const float s = p.sde_lp[b], g = p.gen_lp[b];
        acc[0] += obs + s - g + p.jac[b] + prior - post;
        acc[1] += obs; acc[2] += s; acc[3] += g; acc[4] += prior; acc[5] += post;
    }
    tail_block_sum<6>(red, acc, tid);
    if (tid < 6) p.out[tid] = acc[tid] / (float)p.B;
}

template <bool CNT> __global__ void __launch_bounds__(256) elbo_tail_bwd_kernel(TailParams p, CountLik c) {
    __shared__ float red[256][2 * kTailMaxDim];
    const int tid = threadIdx.x;
    const float ib = 1.f / (float)p.B, g0 = p.g_out[0];
    const float w_obs = (g0 + p.g_out[1]) * ib, w_sde = (g0 + p.g_out[2]) * ib, w_gen = (p.g_out[3] - g0) * ib, w_jac = g0 * ib;
    const float w_prior = (g0 + p.g_out[4]) * ib, w_post = (p.g_out[5] - g0) * ib;
    float gq[2 * kTailMaxDim];
#pragma unroll
    for (int i = 0; i < 2 * kTailMaxDim; ++i) gq[i] = 0.f;
    for (int b = tid; b < p.B; b += 256) {
        tail_obs<true, CNT>(p, c, b, w_obs, XObsRows{p, b});
        p.g_sde[b] = w_sde; p.g_gen[b] = w_gen; p.g_jac[b] = w_jac;
#pragma unroll
        for (int i = 0; i < kTailMaxDim; ++i) {
            if (i < p.P) {
                const float th = p.theta[(int64_t)b * p.P + i];
                const bool pos = (p.theta_pos >> i) & 1u;
                const float lg = (pos || p.prior_lognormal) ? logf(th) : 0.f;
                const float zp = ((p.prior_lognormal ? lg : th) - p.prior_mean) * p.prior_inv_std;
                // d prior / d theta
                float gt = w_prior * (p.prior_lognormal ? (-zp * p.prior_inv_std - 1.f) / th : -zp * p.prior_inv_std);
                const float ls = p.post_log_std[i], e = expf(-ls);
                const float zq = ((pos ? lg : th) - p.post_mean[i]) * e;
                // d post / d theta = d/du (-0.5 zq^2) du/dtheta - [pos] 1/theta
                gt += w_post * (pos ? (-zq * e - 1.f) / th : -zq * e);
                p.g_theta[(int64_t)b * p.P + i] = gt;
                gq[i] += w_post * zq * e;                         // d post / d mean
                gq[kTailMaxDim + i] += w_post * (zq * zq - 1.f);  // d post / d log_std
            }
        }
    }
    tail_block_sum<2 * kTailMaxDim>(red, gq, tid);
    if (tid < p.P) { p.g_post_mean[tid] = gq[tid]; p.g_post_log_std[tid] = gq[kTailMaxDim + tid]; }
}

static int tail_fill(TailParams &p, int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                     const float *obs_matrix, double variance, const float *theta, int prior_type, double prior_mean,
                     double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *theta_positive_mask_host,
                     const float *sde_lp, const float *gen_lp, const float *jac) {
    VSDE_CHECK_ARG(B > 0 && K >= 0 && S > 0 && O > 0 && P > 0, VSDE_E_BADARG, "bad ELBO tail dims B=%d K=%d S=%d O=%d P=%d", B, K, S, O, P);
    VSDE_CHECK_ARG(S <= kTailMaxDim && O <= kTailMaxDim && P <= kTailMaxDim, VSDE_E_BADARG,
                   "ELBO tail kernel supports state / observation / parameter dims <= %d (got %d, %d, %d)", kTailMaxDim, S, O, P);
    VSDE_CHECK_ARG(obs_matrix || O == S, VSDE_E_BADARG, "without an observation matrix obs_dim must equal state_dim (%d vs %d)", O, S);
    VSDE_CHECK_ARG(variance > 0 && prior_std > 0 && (prior_type == 0 || prior_type == 1), VSDE_E_BADARG, "bad variance / prior");
    VSDE_CHECK_ARG((K == 0 || (x_obs && obs_values)) && theta && post_mean && post_log_std && sde_lp && gen_lp && jac, VSDE_E_BADARG,
                   "NULL argument");
    p.B = B; p.K = K; p.S = S; p.O = O; p.P = P; p.x_obs = x_obs; p.obs_values = obs_values; p.obs_matrix = obs_matrix;
    p.inv_var = (float)(1.0 / variance); p.log_norm = (float)(-0.5 * log(2.0 * M_PI * variance));
    p.theta = theta; p.prior_lognormal = prior_type; p.prior_mean = (float)prior_mean; p.prior_inv_std = (float)(1.0 / prior_std);
    p.prior_const = (float)(-log(prior_std) - 0.5 * log(2.0 * M_PI));
    p.post_mean = post_mean; p.post_log_std = post_log_std; p.theta_pos = mask_bits(theta_positive_mask_host, P);
    p.sde_lp = sde_lp; p.gen_lp = gen_lp; p.jac = jac;
    return 0;
}


// ---------------------------------------------------------------------------------------------------------------------
// Importance log-weights of posterior draws (VariationalPosterior.log_evidence): the ELBO integrand of one sample,
//   log w_b = obs_b + sum_t (sde_t - gen_t + jac_t) + prior_b - post_b,
// in one pass over the path.  One workgroup per path, threads striding over t as in elbo_path_terms_kernel; x = softplus(z) on
// the positive state dims and, for the built-in kinds 1..4, drift / diffusion are evaluated in registers (the [B,T,S] /
// [B,T,S,S] coefficient tensors are never written); kind 0 reads the drift / diffusion the caller evaluated.  Each step's
// three terms are summed before the sum over t (no cancellation of two large sums); the sum over t is a fixed tree, and thread
// 0 adds the observation / prior / posterior terms through tail_terms, the per-sample body of the ELBO tail.
struct LogWeightParams {
    TailParams tail;           // observation / prior / posterior (x_obs unused: the states come from z at obs_rows)
    int T;
    const float *z, *means, *chol, *drift, *diffusion;
    const int *obs_rows;       // [K] grid rows of the observations
    uint32_t state_pos;
    float dt, sqdt;
    float *log_w;              // [B]
    CrnNet net;                // kind 4
    const float *rates;        // kind 4 with rate laws: the effective constants [B][2R] of the drift / diffusion
};

// the state of path b at its observed grid points: softplus(z) on the positive dims
template <int S> struct XObsLatent {
    const LogWeightParams &p;
    int b;
    __device__ float operator()(int k, int i) const {
        const int r = min(max(p.obs_rows[k], 0), p.T);
        const float v = p.z[((int64_t)b * (p.T + 1) + r) * S + i];
        return ((p.state_pos >> i) & 1u) ? softplus_f(v) : v;
    }
};

template <int KIND, int S, int NR = EmDims<KIND>::P, bool KIN = false, bool CNT = false>
__global__ void __launch_bounds__(256) log_weight_kernel(LogWeightParams p, CountLik c) {
    constexpr int PK = KIND == 3 ? 2 * S : KIND == 4 ? (KIN ? 2 * NR : NR) : 3;
    const int b = blockIdx.x;
    float th[PK];
    if constexpr (KIN) {
        crn_load_rates<NR>(th, p.rates, b, p.net.R, true);
    } else {
#pragma unroll
        for (int i = 0; i < PK; ++i) th[i] = (KIND == 0 || (KIND == 4 && i >= p.tail.P)) ? 0.f : p.tail.theta[(int64_t)b * p.tail.P + i];
    }
    float acc = 0.f;
    for (int t = threadIdx.x; t < p.T; t += blockDim.x) {
        const int64_t o1 = ((int64_t)b * (p.T + 1) + t) * S, o2 = ((int64_t)b * p.T + t) * S;
        float z0[S], z1[S], x0[S], x1[S], w[S];
#pragma unroll
        for (int i = 0; i < S; ++i) {
            z0[i] = p.z[o1 + i]; z1[i] = p.z[o1 + S + i];
            const bool pos = (p.state_pos >> i) & 1u;
            x0[i] = pos ? softplus_f(z0[i]) : z0[i];
            x1[i] = pos ? softplus_f(z1[i]) : z1[i];
        }
        float sde;
        if constexpr (KIND == 0) {
            sde = tri_logpdf<S>(x1, x0, p.drift + o2, p.diffusion + o2 * S, p.dt, p.sqdt, w);
        } else if constexpr (KIND == 3) {   // f = -a x, G = diag(softplus(b) + 1e-3): the triangular solve is elementwise
            float quad = 0.f, logdet = 0.f;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const float dii = (softplus_f(th[S + i]) + 1e-3f) * p.sqdt;
                const float wi = (x1[i] - (x0[i] + (-th[i] * x0[i]) * p.dt)) / dii;
                quad += wi * wi;
                logdet += __logf(dii);
            }
            sde = -0.5f * ((float)S * kLog2Pi + quad) - logdet;
        } else {
            float f[S], G[S * S];
            if constexpr (KIND == 4) crn_coef<S, NR, KIN>(p.net, x0, th, f, G);
            else coef_fwd<KIND>(x0, th, f, G);
            sde = tri_logpdf<S>(x1, x0, f, G, p.dt, p.sqdt, w);
        }
        const float gen = tri_logpdf<S>(z1, z0, p.means + o2, p.chol + o2 * S, p.dt, p.sqdt, w);
        float jac = 0.f;
#pragma unroll
        for (int i = 0; i < S; ++i)
            if ((p.state_pos >> i) & 1u) jac += log_sigmoid(z1[i]);
        acc += sde - gen + jac;
    }
    __shared__ float red[4];
    acc = wave_sum(acc);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float path = 0.f;
        for (int i = 0; i < (int)(blockDim.x >> 6); ++i) path += red[i];
        const TailTerms tt = tail_terms<CNT>(p.tail, c, b, XObsLatent<S>{p, b});
        p.log_w[b] = tt.obs + path + tt.prior - tt.post;
    }
}

// c: the count observation term (its Gaussian instantiation when c is NULL)
template <int KIND, int S, int NR = EmDims<KIND>::P, bool KIN = false>
static int launch_log_weights(const LogWeightParams &p, hipStream_t s, const CountLik *c = nullptr) {
    if (c) hipLaunchKernelGGL((log_weight_kernel<KIND, S, NR, KIN, true>), dim3(p.tail.B), dim3(256), 0, s, p, *c);
    else hipLaunchKernelGGL((log_weight_kernel<KIND, S, NR, KIN, false>), dim3(p.tail.B), dim3(256), 0, s, p, CountLik{});
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

// Streamed reduction of log-weights into a running fp64 state
//   state = [M, sum exp(lw - M), sum exp(2 (lw - M)), sum lw, n, n_nonfinite]
// One workgroup per chunk: chunk max, then the chunk sums against it (thread-strided, then a fixed LDS tree: the same draws give
// the same bits), merged into the state by rescaling both sides to the new max.  NaN and +inf weights are counted in n_nonfinite
// and left out of the sums; -inf weights are zero weights and count in n only.
__device__ __forceinline__ bool lw_finite(float v) { return v == v && v != INFINITY; }

__global__ void __launch_bounds__(256) log_weight_accumulate_kernel(int n, const float *__restrict__ lw, double *__restrict__ st) {
    __shared__ double red[256][4];
    const int tid = threadIdx.x;
    float m = -INFINITY;
    double bad = 0.0;
    for (int i = tid; i < n; i += 256) {
        const float v = lw[i];
        if (lw_finite(v)) m = fmaxf(m, v);
        else bad += 1.0;
    }
    red[tid][0] = m; red[tid][1] = bad;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) { red[tid][0] = fmax(red[tid][0], red[tid + w][0]); red[tid][1] += red[tid + w][1]; }
        __syncthreads();
    }
    const double mc = red[0][0], nbad = red[0][1];
    __syncthreads();
    double v[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
        const float x = lw[i];
        if (!lw_finite(x)) continue;
        if (mc > -INFINITY) {
            const double e = exp((double)x - mc);
            v[0] += e; v[1] += e * e;
        }
        v[2] += (double)x;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) red[tid][j] = v[j];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w)
#pragma unroll
            for (int j = 0; j < 3; ++j) red[tid][j] += red[tid + w][j];
        __syncthreads();
    }
    if (tid == 0) {
        const double m0 = st[0], mn = fmax(m0, mc);
        const double a = mn > -INFINITY ? exp(m0 - mn) : 0.0, c = mn > -INFINITY ? exp(mc - mn) : 0.0;
        st[0] = mn;
        st[1] = st[1] * a + red[0][0] * c;
        st[2] = st[2] * (a * a) + red[0][1] * (c * c);
        st[3] += red[0][2];
        st[4] += (double)n;
        st[5] += nbad;
    }
}

}  // namespace vsde

using namespace vsde;

extern "C" int vsde_elbo_path_terms(int B, int T, int S, const float *z, const float *x, const float *means,
                                    const float *chol, const float *drift, const float *diffusion,
                                    const uint8_t *positive_mask_host, double time_step, float *sde_lp,
                                    float *gen_lp, float *log_jac, void *stream) {
    VSDE_CHECK_ARG(B > 0 && T > 0 && S > 0, VSDE_E_BADARG, "bad dims B=%d T=%d S=%d", B, T, S);
    VSDE_CHECK_ARG(z && x && means && chol && drift && diffusion && sde_lp && gen_lp && log_jac, VSDE_E_BADARG, "NULL argument");
    ElboParams p = {};
    p.B = B; p.T = T; p.z = z; p.x = x; p.means = means; p.chol = chol; p.drift = drift; p.diffusion = diffusion;
    p.pos_mask = mask_bits(positive_mask_host, S); p.dt = (float)time_step; p.sqdt = (float)sqrt(time_step);
    p.sde_lp = sde_lp; p.gen_lp = gen_lp; p.jac = log_jac;
    return dispatch_elbo(S, p, false, (hipStream_t)stream);
}

extern "C" int vsde_elbo_path_terms_bwd(int B, int T, int S, const float *z, const float *x, const float *means,
                                        const float *chol, const float *drift, const float *diffusion,
                                        const uint8_t *positive_mask_host, double time_step, const float *g_sde,
                                        const float *g_gen, const float *g_jac, float *g_z, float *g_x,
                                        float *g_means, float *g_chol, float *g_drift, float *g_diffusion,
                                        void *stream) {
    VSDE_CHECK_ARG(B > 0 && T > 0 && S > 0, VSDE_E_BADARG, "bad dims B=%d T=%d S=%d", B, T, S);
    VSDE_CHECK_ARG(z && x && means && chol && drift && diffusion && g_sde && g_gen && g_jac && g_z && g_x && g_means && g_chol &&
                       g_drift && g_diffusion, VSDE_E_BADARG, "NULL argument");
    // the backward puts b on gridDim.y
    VSDE_CHECK_ARG(B <= kElboBwdMaxPaths, VSDE_E_BADARG, "ELBO path-term backward supports at most %d paths per call (got %d)",
                   kElboBwdMaxPaths, B);
    ElboParams p = {};
    p.B = B; p.T = T; p.z = z; p.x = x; p.means = means; p.chol = chol; p.drift = drift; p.diffusion = diffusion;
    p.pos_mask = mask_bits(positive_mask_host, S); p.dt = (float)time_step; p.sqdt = (float)sqrt(time_step);
    p.g_sde = g_sde; p.g_gen = g_gen; p.g_jac = g_jac;
    p.g_z = g_z; p.g_x = g_x; p.g_means = g_means; p.g_chol = g_chol; p.g_drift = g_drift; p.g_diffusion = g_diffusion;
    return dispatch_elbo(S, p, true, (hipStream_t)stream);
}

static int tail_fwd(const CountArgs *ca, int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                    const float *obs_matrix, double variance, const float *theta, int prior_type, double prior_mean,
                    double prior_std, const float *post_mean, const float *post_log_std,
                    const uint8_t *theta_positive_mask_host, const float *sde_lp, const float *gen_lp,
                    const float *log_jac, float *out6, void *stream) {
    TailParams p = {};
    CountLik c = {};
    int rc = tail_fill(p, B, K, S, O, P, x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std, post_mean,
                       post_log_std, theta_positive_mask_host, sde_lp, gen_lp, log_jac);
    if (rc) return rc;
    VSDE_CHECK_ARG(out6, VSDE_E_BADARG, "NULL output");
    if ((rc = count_fill(c, ca, K))) return rc;
    p.out = out6;
    if (ca) hipLaunchKernelGGL(elbo_tail_fwd_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, p, c);
    else hipLaunchKernelGGL(elbo_tail_fwd_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, p, c);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int vsde_elbo_tail_fwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                                  const float *obs_matrix, double variance, const float *theta, int prior_type, double prior_mean,
                                  double prior_std, const float *post_mean, const float *post_log_std,
                                  const uint8_t *theta_positive_mask_host, const float *sde_lp, const float *gen_lp,
                                  const float *log_jac, float *out6, void *stream) {
    return tail_fwd(nullptr, B, K, S, O, P, x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std,
                    post_mean, post_log_std, theta_positive_mask_host, sde_lp, gen_lp, log_jac, out6, stream);
}

extern "C" int vsde_count_elbo_tail_fwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                                        const float *obs_matrix, int lik_kind, double scale, double dispersion,
                                        const float *row_const, const float *theta, int prior_type, double prior_mean,
                                        double prior_std, const float *post_mean, const float *post_log_std,
                                        const uint8_t *theta_positive_mask_host, const float *sde_lp, const float *gen_lp,
                                        const float *log_jac, float *out6, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return tail_fwd(&ca, B, K, S, O, P, x_obs, obs_values, obs_matrix, 1.0, theta, prior_type, prior_mean, prior_std, post_mean,
                    post_log_std, theta_positive_mask_host, sde_lp, gen_lp, log_jac, out6, stream);
}

static int tail_bwd(const CountArgs *ca, int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                    const float *obs_matrix, double variance, const float *theta, int prior_type, double prior_mean,
                    double prior_std, const float *post_mean, const float *post_log_std,
                    const uint8_t *theta_positive_mask_host, const float *g_out6, float *g_x_obs, float *g_theta,
                    float *g_post_mean, float *g_post_log_std, float *g_sde, float *g_gen, float *g_jac, void *stream) {
    TailParams p = {};
    CountLik c = {};
    // the path-term inputs are not read by the backward: any non-NULL pointer satisfies the shared argument check
    int rc = tail_fill(p, B, K, S, O, P, x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std, post_mean,
                       post_log_std, theta_positive_mask_host, theta, theta, theta);
    if (rc) return rc;
    VSDE_CHECK_ARG(g_out6 && (K == 0 || g_x_obs) && g_theta && g_post_mean && g_post_log_std && g_sde && g_gen && g_jac, VSDE_E_BADARG,
                   "NULL argument");
    p.g_out = g_out6; p.g_x_obs = g_x_obs; p.g_theta = g_theta; p.g_post_mean = g_post_mean; p.g_post_log_std = g_post_log_std;
    if ((rc = count_fill(c, ca, K))) return rc;
    p.g_sde = g_sde; p.g_gen = g_gen; p.g_jac = g_jac;
    if (ca) hipLaunchKernelGGL(elbo_tail_bwd_kernel<true>, dim3(1), dim3(256), 0, (hipStream_t)stream, p, c);
    else hipLaunchKernelGGL(elbo_tail_bwd_kernel<false>, dim3(1), dim3(256), 0, (hipStream_t)stream, p, c);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int vsde_elbo_tail_bwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                                  const float *obs_matrix, double variance, const float *theta, int prior_type, double prior_mean,
                                  double prior_std, const float *post_mean, const float *post_log_std,
                                  const uint8_t *theta_positive_mask_host, const float *g_out6, float *g_x_obs, float *g_theta,
                                  float *g_post_mean, float *g_post_log_std, float *g_sde, float *g_gen, float *g_jac, void *stream) {
    return tail_bwd(nullptr, B, K, S, O, P, x_obs, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std,
                    post_mean, post_log_std, theta_positive_mask_host, g_out6, g_x_obs, g_theta, g_post_mean, g_post_log_std, g_sde,
                    g_gen, g_jac, stream);
}

extern "C" int vsde_count_elbo_tail_bwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values,
                                        const float *obs_matrix, int lik_kind, double scale, double dispersion,
                                        const float *row_const, const float *theta, int prior_type, double prior_mean,
                                        double prior_std, const float *post_mean, const float *post_log_std,
                                        const uint8_t *theta_positive_mask_host, const float *g_out6, float *g_x_obs,
                                        float *g_theta, float *g_post_mean, float *g_post_log_std, float *g_sde, float *g_gen,
                                        float *g_jac, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return tail_bwd(&ca, B, K, S, O, P, x_obs, obs_values, obs_matrix, 1.0, theta, prior_type, prior_mean, prior_std, post_mean,
                    post_log_std, theta_positive_mask_host, g_out6, g_x_obs, g_theta, g_post_mean, g_post_log_std, g_sde, g_gen,
                    g_jac, stream);
}


// rt.kind 0: the caller's drift / diffusion tensors; 1..4: the route's own.  P is the dim of theta (prior / posterior terms) and PM
// the route's parameter dim: P, or with rate laws the effective constants' 2R (`rates`; NULL on the other routes)
static int log_weights_impl(const CountArgs *ca, const SdeRoute &rt, int B, int T, int S, int K, int O, int P, int PM, const float *z, const float *means, const float *chol, const float *drift, const float *diffusion, const float *theta, const float *rates, const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    LogWeightParams p = {};
    // a network's descriptors fix S, so their checks come first; the built-in kinds' relations come after the kernel's own dims
    // (S beyond its 16: VSDE_E_STATE)
    int rc = rt.descriptors ? crn_route_net(rt, S, PM, p.net) : 0;
    if (rc) return rc;
    VSDE_CHECK_ARG(B > 0 && T > 0 && S > 0 && K >= 0, VSDE_E_BADARG, "bad log-weight dims B=%d T=%d S=%d K=%d", B, T, S, K);
    VSDE_CHECK_ARG(S <= kTailMaxDim, VSDE_E_STATE, "state_dim %d not supported by the log-weight kernel (1..%d)", S, kTailMaxDim);
    VSDE_CHECK_ARG(rt.descriptors || (rt.kind >= 0 && rt.kind <= 3), VSDE_E_BADARG, "unknown SDE kind %d (0 = caller's coefficients, 1..3 built in)", rt.kind);
    if (!rt.descriptors && rt.kind && (rc = kind_check(rt.kind, S, PM))) return rc;
    VSDE_CHECK_ARG(rt.kind != 0 || (drift && diffusion), VSDE_E_BADARG, "kind 0 needs the drift and diffusion tensors");
    VSDE_CHECK_ARG(z && means && chol && (rates || rt.descriptors < 2) && log_w && (K == 0 || obs_rows) && time_step > 0, VSDE_E_BADARG,
                   "NULL argument / bad time_step");
    // the tail's x_obs and path-term inputs are not read here (the states come from z): any non-NULL pointer passes its check
    rc = tail_fill(p.tail, B, K, S, O, P, z, obs_values, obs_matrix, variance, theta, prior_type, prior_mean, prior_std,
                   post_mean, post_log_std, theta_positive_mask_host, z, z, z);
    if (rc) return rc;
    CountLik c = {};
    if ((rc = count_fill(c, ca, K))) return rc;
    p.T = T; p.z = z; p.means = means; p.chol = chol; p.drift = drift; p.diffusion = diffusion; p.obs_rows = obs_rows; p.rates = rates;
    p.state_pos = mask_bits(state_positive_mask_host, S); p.dt = (float)time_step; p.sqdt = (float)sqrt(time_step); p.log_w = log_w;
    const auto launch = [&](auto kind, auto ns, auto nr, auto kin) {
        return launch_log_weights<decltype(kind)::value, decltype(ns)::value, decltype(nr)::value, decltype(kin)::value>(p, (hipStream_t)stream, ca ? &c : nullptr);
    };
    if (rt.kind == 0) return dispatch_dim<kTailMaxDim>(S, [&](auto ns) { return launch(IntC<0>{}, ns, IntC<EmDims<0>::P>{}, std::false_type{}); });
    return route_dispatch<kTailMaxDim>(rt, S, p.net.R, launch);
}

extern "C" int vsde_log_weights(int kind, int B, int T, int S, int K, int O, int P, const float *z, const float *means, const float *chol, const float *drift, const float *diffusion, const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    return log_weights_impl(nullptr, SdeRoute{kind}, B, T, S, K, O, P, P, z, means, chol, drift, diffusion, theta, nullptr, obs_rows, obs_values, obs_matrix, variance, prior_type, prior_mean, prior_std, post_mean, post_log_std, state_positive_mask_host, theta_positive_mask_host, time_step, log_w, stream);
}

extern "C" int vsde_count_log_weights(int kind, int B, int T, int S, int K, int O, int P, const float *z, const float *means, const float *chol, const float *drift, const float *diffusion, const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix, int lik_kind, double scale, double dispersion, const float *row_const, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return log_weights_impl(&ca, SdeRoute{kind}, B, T, S, K, O, P, P, z, means, chol, drift, diffusion, theta, nullptr, obs_rows, obs_values, obs_matrix, 1.0, prior_type, prior_mean, prior_std, post_mean, post_log_std, state_positive_mask_host, theta_positive_mask_host, time_step, log_w, stream);
}

extern "C" int vsde_log_weight_accumulate(int n, const float *log_w, double *state6, void *stream) {
    VSDE_CHECK_ARG(n > 0, VSDE_E_BADARG, "log-weight count must be positive (got %d)", n);
    VSDE_CHECK_ARG(log_w && state6, VSDE_E_BADARG, "NULL argument");
    hipLaunchKernelGGL(log_weight_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n, log_w, state6);
    VSDE_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int vsde_crn_log_weights(const vsde_crn_network *net, int B, int T, int S, int K, int O, int P, const float *z, const float *means, const float *chol, const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    return log_weights_impl(nullptr, crn_route(net), B, T, S, K, O, P, P, z, means, chol, nullptr, nullptr, theta, nullptr, obs_rows, obs_values, obs_matrix, variance, prior_type, prior_mean, prior_std, post_mean, post_log_std, state_positive_mask_host, theta_positive_mask_host, time_step, log_w, stream);
}

extern "C" int vsde_crn_count_log_weights(const vsde_crn_network *net, int B, int T, int S, int K, int O, int P, const float *z, const float *means, const float *chol, const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix, int lik_kind, double scale, double dispersion, const float *row_const, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return log_weights_impl(&ca, crn_route(net), B, T, S, K, O, P, P, z, means, chol, nullptr, nullptr, theta, nullptr, obs_rows, obs_values, obs_matrix, 1.0, prior_type, prior_mean, prior_std, post_mean, post_log_std, state_positive_mask_host, theta_positive_mask_host, time_step, log_w, stream);
}

extern "C" int vsde_crn_kinetic_log_weights(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int K, int O, int P, int R_eff, const float *z, const float *means, const float *chol, const float *theta, const float *rates, const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    return log_weights_impl(nullptr, crn_route(net, kin), B, T, S, K, O, P, R_eff, z, means, chol, nullptr, nullptr, theta, rates, obs_rows, obs_values, obs_matrix, variance, prior_type, prior_mean, prior_std, post_mean, post_log_std, state_positive_mask_host, theta_positive_mask_host, time_step, log_w, stream);
}

extern "C" int vsde_crn_kinetic_count_log_weights(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int K, int O, int P, int R_eff, const float *z, const float *means, const float *chol, const float *theta, const float *rates, const int *obs_rows, const float *obs_values, const float *obs_matrix, int lik_kind, double scale, double dispersion, const float *row_const, int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream) {
    const CountArgs ca = {lik_kind, scale, dispersion, row_const};
    return log_weights_impl(&ca, crn_route(net, kin), B, T, S, K, O, P, R_eff, z, means, chol, nullptr, nullptr, theta, rates, obs_rows, obs_values, obs_matrix, 1.0, prior_type, prior_mean, prior_std, post_mean, post_log_std, state_positive_mask_host, theta_positive_mask_host, time_step, log_w, stream);
}
