// Drift / diffusion of the SDEs built into the library, as device functions shared by the simulator and the coefficient kernels
// (vsde_sde.hip) and the importance log-weight kernel (vsde_elbo.hip), so the closed forms exist once:
//   kind 1  Ornstein-Uhlenbeck  (examples/ornstein_uhlenbeck.py:18-30)   f = kappa (mu - x),   G = sigma
//   kind 2  Lotka-Volterra      (examples/lotka_volterra.py:18-46)       analytic 2x2 Cholesky factor, three clamp(min=1e-6)
//   kind 3  linear / diagonal   (BASELINE config 5)                       f = -a x, G = diag(softplus(b) + 1e-3)
//   kind 4  reaction network    (core/reaction_network.py)                mass action or Hill rate laws, floored Cholesky factor of
//                                                                         sum_j h_j nu_j nu_j^T
#pragma once
#include <type_traits>

#include "vsde_common.h"

namespace vsde {

constexpr float kEmFloor = 1e-6f;
// clamp(min = 1e-6) that propagates NaN like torch.clamp / torch.maximum do (fmaxf(NaN, floor) would return the floor and hide a
// diverged path from the non-finite-loss guards of the pre-training loop and the ELBO)
__device__ __forceinline__ float floor_nan(float y) { return y < kEmFloor ? kEmFloor : y; }

constexpr int kCrnMaxS = VSDE_CRN_MAX_SPECIES, kCrnMaxR = VSDE_CRN_MAX_REACTIONS;

// Count observation terms (core/observations.py: PoissonObservationLikelihood / NegativeBinomialObservationLikelihood), shared by
// the ELBO tail, the log-weight and the particle-filter kernels.  lambda = max(scale pred, kRateFloor) with torch.clamp's rules (NaN
// propagates, the gradient is 0 where scale pred < floor).  The terms of y alone (lgamma's, r log r, y log y) arrive as one float
// per observation row (row_const [K], made in fp64 by the caller); the kernel adds the deviance form, which is O((lambda - y)^2 / y)
// near lambda = y where the raw form cancels y log(lambda) against a constant of the same size:
//   Poisson  y log(lambda / y) - (lambda - y)                                       (y = 0: -lambda)
//   NB       y log(lambda / y) - (r + y) log((r + lambda) / (r + y))                (y = 0: -r log((r + lambda) / r))
// with log(a / b) = log1p((a - b) / b) while a is within a factor 2 of b (a - b is then exact).
constexpr float kRateFloor = 1e-6f;   // core/observations.py: RATE_FLOOR
struct CountLik {
    int kind;                  // VSDE_LIK_POISSON / VSDE_LIK_NEGATIVE_BINOMIAL
    float scale, r;            // r: the dispersion (NB only)
    const float *row_const;    // [K]
};

// the count entry points' own argument checks (K: the number of observation rows)
static inline int count_lik(CountLik &c, int lik_kind, double scale, double dispersion, const float *row_const, int K) {
    VSDE_CHECK_ARG(lik_kind == VSDE_LIK_POISSON || lik_kind == VSDE_LIK_NEGATIVE_BINOMIAL, VSDE_E_BADARG,
                   "unknown count likelihood %d (1 = Poisson, 2 = negative binomial)", lik_kind);
    VSDE_CHECK_ARG(scale > 0, VSDE_E_BADARG, "count likelihood: scale must be positive");
    VSDE_CHECK_ARG(lik_kind != VSDE_LIK_NEGATIVE_BINOMIAL || dispersion > 0, VSDE_E_BADARG,
                   "negative binomial: dispersion must be positive");
    VSDE_CHECK_ARG(row_const || K == 0, VSDE_E_BADARG, "count likelihood: NULL row constants");
    c.kind = lik_kind; c.scale = (float)scale; c.r = lik_kind == VSDE_LIK_NEGATIVE_BINOMIAL ? (float)dispersion : 1.f;
    c.row_const = row_const;
    return 0;
}

// the count arguments of a vsde_*count_* entry point (NULL: the Gaussian form); checked after the shared checks
struct CountArgs { int lik_kind; double scale, dispersion; const float *row_const; };
static inline int count_fill(CountLik &c, const CountArgs *ca, int K) {
    return ca ? count_lik(c, ca->lik_kind, ca->scale, ca->dispersion, ca->row_const, K) : 0;
}

__device__ __forceinline__ float log_ratio(float a, float b) {
    const float d = a - b;
    return fabsf(d) < 0.5f * b ? log1pf(d / b) : logf(a / b);
}

// the deviance term of one observed count y at the linear prediction pred; dlam: d term / d pred (0 where the floor binds)
template <bool GRAD> __device__ __forceinline__ float count_term(const CountLik &c, float y, float pred, float &dpred) {
    const float sp = c.scale * pred;
    const float lam = sp < kRateFloor ? kRateFloor : sp;
    float t;
    if (c.kind == VSDE_LIK_POISSON) {
        t = y > 0.f ? y * log_ratio(lam, y) - (lam - y) : -lam;
        if (GRAD) dpred = sp < kRateFloor ? 0.f : c.scale * (y - lam) / lam;
    } else {
        const float ry = c.r + y;
        t = -ry * log_ratio(c.r + lam, ry);
        if (y > 0.f) t += y * log_ratio(lam, y);
        if (GRAD) dpred = sp < kRateFloor ? 0.f : c.scale * c.r * (y - lam) / (lam * (c.r + lam));
    }
    return t;
}

// state / parameter dims of the fixed-size kinds (kind 3 takes them at run time; the value here is its per-dimension slice; kind 4
// takes S and the reaction bound NR as template arguments of its kernels, R <= NR at run time: P = NR sizes its theta array)
template <int KIND> struct EmDims {
    static constexpr int S = KIND == 2 ? 2 : 1;
    static constexpr int P = KIND == 3 ? 2 : KIND == 4 ? kCrnMaxR : 3;
};

// F.softplus (threshold 20)
__device__ __forceinline__ float softplus_f(float b) { return b > 20.f ? b : log1pf(__expf(b)); }

// drift f [S] and diffusion factor G [S][S] (row-major, lower triangular) of kinds 1, 2 at state x
template <int KIND> __device__ __forceinline__ void coef_fwd(const float *x, const float *th, float *f, float *G) {
    if constexpr (KIND == 1) {
        f[0] = th[0] * (th[1] - x[0]); G[0] = th[2];
    } else {
        const float u = x[0], v = x[1], uv = th[1] * u * v;
        const float l00 = sqrtf(floor_nan(th[0] * u + uv));
        const float l10 = -uv / floor_nan(l00);
        const float l11 = sqrtf(floor_nan(th[2] * v + uv - l10 * l10));
        f[0] = th[0] * u - uv; f[1] = uv - th[2] * v;
        G[0] = l00; G[1] = 0.f; G[2] = l10; G[3] = l11;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Kind 4: mass-action reaction network (include/vsde_hip.h: vsde_crn_network).  S is a template argument, R <= kCrnMaxR is read at
// run time.  The network travels by value in the kernel's parameter struct; every loop over reactions is unrolled to the bound
// NR (a template argument: 4, 8 or 16, the smallest that holds R) under a uniform `j < R` guard, so the tables are read at
// compile-time offsets of the kernel arguments (scalar loads) and theta_j and the per-reaction values stay in registers: an array
// indexed by a run-time j would go to scratch.  The bound keeps the table entries a small network needs, not all 16 rows, in SGPRs.
struct CrnNet {
    int R;
    int8_t order[kCrnMaxR][kCrnMaxS];   // reactant orders, 0..3
    float change[kCrnMaxR][kCrnMaxS];   // net change as float: FMA operands straight from the kernel arguments
    // rate laws (vsde_crn_kinetics): read only by the KIN instantiations, zero for the mass-action entry points
    int8_t law[kCrnMaxR], mod[kCrnMaxR], hill_n[kCrnMaxR];
};

// validate a C-ABI descriptor (host memory) against the call's S / P and convert it into the kernel-argument form; P is R, or 2R
// for the rate-law entry points (kinetic: theta is the effective constants (k_0 .. k_{R-1}, K_0 .. K_{R-1}))
static inline int crn_net(const vsde_crn_network *d, int S, int P, CrnNet &n, bool kinetic = false) {
    VSDE_CHECK_ARG(d, VSDE_E_BADARG, "NULL reaction-network descriptor");
    VSDE_CHECK_ARG(d->S >= 1 && d->S <= kCrnMaxS, VSDE_E_BADARG, "reaction network: %d species (1..%d supported)", d->S, kCrnMaxS);
    VSDE_CHECK_ARG(d->R >= 1 && d->R <= kCrnMaxR, VSDE_E_BADARG, "reaction network: %d reactions (1..%d supported)", d->R, kCrnMaxR);
    for (int j = 0; j < d->R; ++j)
        for (int i = 0; i < d->S; ++i)
            VSDE_CHECK_ARG(d->order[j][i] >= 0 && d->order[j][i] <= VSDE_CRN_MAX_ORDER, VSDE_E_BADARG,
                           "reaction network: reaction %d has order %d in species %d (0..%d supported)", j, (int)d->order[j][i], i,
                           VSDE_CRN_MAX_ORDER);
    if (kinetic)
        VSDE_CHECK_ARG(S == d->S && P == 2 * d->R, VSDE_E_BADARG,
                       "reaction network of %d species and %d reactions called with state_dim %d and %d effective constants (2R = %d)",
                       d->S, d->R, S, P, 2 * d->R);
    else
        VSDE_CHECK_ARG(S == d->S && P == d->R, VSDE_E_BADARG,
                       "reaction network of %d species and %d reactions called with state_dim %d, sde_param_dim %d", d->S, d->R, S, P);
    n = CrnNet{};
    n.R = d->R;
    for (int j = 0; j < d->R; ++j)
        for (int i = 0; i < d->S; ++i) { n.order[j][i] = d->order[j][i]; n.change[j][i] = (float)d->change[j][i]; }
    return 0;
}

// validate a rate-law descriptor (host memory) against the network already in n (crn_net first) and copy it into n
static inline int crn_kinetics(const vsde_crn_kinetics *k, int S, CrnNet &n) {
    VSDE_CHECK_ARG(k, VSDE_E_BADARG, "NULL rate-law descriptor");
    for (int j = 0; j < n.R; ++j) {
        const int law = k->law[j];
        VSDE_CHECK_ARG(law >= VSDE_CRN_LAW_MASS_ACTION && law <= VSDE_CRN_LAW_HILL_REPRESSION, VSDE_E_BADARG,
                       "rate laws: reaction %d has law code %d (0..2 supported)", j, law);
        if (law == VSDE_CRN_LAW_MASS_ACTION) continue;
        VSDE_CHECK_ARG(k->modifier[j] >= 0 && k->modifier[j] < S, VSDE_E_BADARG,
                       "rate laws: reaction %d has modifier species %d (0..%d for %d species)", j, (int)k->modifier[j], S - 1, S);
        VSDE_CHECK_ARG(k->hill_n[j] >= 1 && k->hill_n[j] <= VSDE_CRN_MAX_HILL, VSDE_E_BADARG,
                       "rate laws: reaction %d has Hill coefficient %d (1..%d supported)", j, (int)k->hill_n[j], VSDE_CRN_MAX_HILL);
    }
    for (int j = 0; j < n.R; ++j) {
        const bool ma = k->law[j] == VSDE_CRN_LAW_MASS_ACTION;
        n.law[j] = k->law[j]; n.mod[j] = ma ? 0 : k->modifier[j]; n.hill_n[j] = ma ? 1 : k->hill_n[j];
    }
    return 0;
}

// x^r by repeated multiplication (r uniform, 0..3) and its derivative r x^(r-1)
__device__ __forceinline__ float crn_pow(float x, int r) { return r == 0 ? 1.f : r == 1 ? x : r == 2 ? x * x : x * x * x; }
__device__ __forceinline__ float crn_dpow(float x, int r) { return r == 0 ? 0.f : r == 1 ? 1.f : r == 2 ? 2.f * x : 3.f * (x * x); }

// a rate-law table entry as an opaque uniform value.  Read plainly, the entries of all NR reactions are loop-invariant in the time
// loops, and the compiler hoists every comparison made with them (law, Hill coefficient, `i == s`: each a 64-lane mask, 2 SGPRs)
// out of the loop: 100-800 SGPRs spilled to VGPR lanes, and scratch.  The empty asm makes each read a fresh value and the
// (convergent, so never hoisted) readfirstlane returns it to an SGPR as a uniform value: the masks are remade next to their use,
// a few instructions per reaction and step.
__device__ __forceinline__ int crn_rl(int v) {
    asm volatile("" : "+v"(v));
    return __builtin_amdgcn_readfirstlane(v);
}

// v^e for a Hill coefficient e (uniform, 1..4) by repeated multiplication, ((v v) v) v: the spec's operation order
__device__ __forceinline__ float crn_hpow(float v, int e) {
    float r = v;
#pragma unroll
    for (int k = 1; k < VSDE_CRN_MAX_HILL; ++k)
        if (k < e) r *= v;
    return r;
}

// x[s] for a uniform run-time s: an unrolled select over the S registers (indexing the array by s would put it in scratch)
template <int S> __device__ __forceinline__ float crn_pick(const float *x, int s) {
    float v = 0.f;
#pragma unroll
    for (int i = 0; i < S; ++i)
        if (i == s) v = x[i];
    return v;
}

// propensity h_j; th [NR] = k (mass action only), or [2 NR] = (k, K) with KIN (rate laws: u = clamp(x_s, min=0), a = u^n,
// c = K^n, g = a / (c + a) or c / (c + a), h = k g; `u` keeps NaN like torch.clamp)
template <int S, int NR, bool KIN>
__device__ __forceinline__ float crn_propensity(const CrnNet &n, int j, const float *x, const float *th) {
    if constexpr (KIN) {
        const int law = crn_rl(n.law[j]);
        if (law != VSDE_CRN_LAW_MASS_ACTION) {
            const int e = crn_rl(n.hill_n[j]);
            const float xs = crn_pick<S>(x, crn_rl(n.mod[j])), u = xs < 0.f ? 0.f : xs;
            const float a = crn_hpow(u, e), c = crn_hpow(th[NR + j], e);
            return th[j] * ((law == VSDE_CRN_LAW_HILL_ACTIVATION ? a : c) / (c + a));
        }
    }
    float m = 1.f;
#pragma unroll
    for (int i = 0; i < S; ++i) m *= crn_pow(x[i], n.order[j][i]);
    return th[j] * m;
}

// propensity a_j of the jump process (core/jump_process.py) at the integer state xi [S], xf = (float)xi: mass action with the
// falling factorial x (x - 1) .. (x - r + 1) in place of x^r (0 once x < r); a rate law as in crn_propensity with u = x_s (never
// negative here), times the gate 1[x_i >= r_ji for all i]: its reactant row still consumes.  `orders` is the reaction's reactant
// row packed 2 bits per species (crn_pack_orders), one opaque uniform word per reaction and event (crn_rl): the 3 S comparisons
// made with a plain table entry are loop-invariant in the event loop and their masks would be hoisted into spilled SGPRs.
template <int S, int NR, bool KIN>
__device__ __forceinline__ float crn_jump_propensity(const CrnNet &n, uint32_t orders, int j, const int *xi, const float *xf,
                                                     const float *th) {
    orders = (uint32_t)crn_rl((int)orders);
    if constexpr (KIN) {
        const int law = crn_rl(n.law[j]);
        if (law != VSDE_CRN_LAW_MASS_ACTION) {
            const int e = crn_rl(n.hill_n[j]);
            const float u = crn_pick<S>(xf, crn_rl(n.mod[j]));
            const float a = crn_hpow(u, e), c = crn_hpow(th[NR + j], e);
            bool open = true;
#pragma unroll
            for (int i = 0; i < S; ++i) open = open && xi[i] >= (int)((orders >> (2 * i)) & 3u);
            return th[j] * ((law == VSDE_CRN_LAW_HILL_ACTIVATION ? a : c) / (c + a)) * (open ? 1.f : 0.f);
        }
    }
    float m = 1.f;
#pragma unroll
    for (int i = 0; i < S; ++i) {
        const uint32_t r = (orders >> (2 * i)) & 3u;
        if (r >= 1u) m *= xf[i];
        if (r >= 2u) m *= xf[i] - 1.f;
        if (r >= 3u) m *= xf[i] - 2.f;
    }
    return th[j] * m;
}

// host: a descriptor's reactant row (orders 0..3, already checked by crn_net) packed 2 bits per species
static inline uint32_t crn_pack_orders(const vsde_crn_network *d, int j) {
    uint32_t w = 0;
    for (int i = 0; i < d->S; ++i) w |= (uint32_t)d->order[j][i] << (2 * i);
    return w;
}

// drift f [S] and the lower triangle of Sigma = sum_j h_j nu_j nu_j^T in sig [S][S]
template <int S, int NR, bool KIN = false>
__device__ __forceinline__ void crn_drift_cov(const CrnNet &n, const float *x, const float *th, float *f, float *sig) {
#pragma unroll
    for (int i = 0; i < S; ++i) {
        f[i] = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) sig[i * S + k] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j < n.R) {
            const float h = crn_propensity<S, NR, KIN>(n, j, x, th);
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const float hn = h * n.change[j][i];
                f[i] += hn;
#pragma unroll
                for (int k = 0; k <= i; ++k) sig[i * S + k] += hn * n.change[j][k];
            }
        }
    }
}

// in place: the lower triangle of Sigma in a [S][S] -> its floored Cholesky factor (upper triangle zeroed); sd[j] = the diagonal
// quantity before its floor (the backward's clamp test)
template <int S> __device__ __forceinline__ void crn_chol(float *a, float *sd) {
#pragma unroll
    for (int j = 0; j < S; ++j) {
        float s = a[j * S + j];
#pragma unroll
        for (int k = 0; k < j; ++k) s -= a[j * S + k] * a[j * S + k];
        sd[j] = s;
        const float ljj = sqrtf(floor_nan(s)), c = floor_nan(ljj);
        a[j * S + j] = ljj;
#pragma unroll
        for (int i = j + 1; i < S; ++i) {
            float v = a[i * S + j];
#pragma unroll
            for (int k = 0; k < j; ++k) v -= a[i * S + k] * a[j * S + k];
            a[i * S + j] = v / c;
            a[j * S + i] = 0.f;
        }
    }
}

// drift f [S] and diffusion factor G [S][S] (row-major, lower triangular) of a network at state x; th [NR] ([2 NR] with KIN)
template <int S, int NR, bool KIN = false>
__device__ __forceinline__ void crn_coef(const CrnNet &n, const float *x, const float *th, float *f, float *G) {
    float sd[S];
    crn_drift_cov<S, NR, KIN>(n, x, th, f, G);
    crn_chol<S>(G, sd);
}

// vector-Jacobian product of crn_coef: (gf [S], lower triangle of gG [S][S]) -> gx [S] (overwritten), gth [NR] ([2 NR] with KIN)
// (+=)
template <int S, int NR, bool KIN = false>
__device__ __forceinline__ void crn_coef_bwd(const CrnNet &n, const float *x, const float *th, const float *gf, const float *gG,
                                             float *gx, float *gth) {
    float f[S], L[S * S], sd[S], d[S * S];
    crn_drift_cov<S, NR, KIN>(n, x, th, f, L);
    crn_chol<S>(L, sd);
#pragma unroll
    for (int i = 0; i < S; ++i) {
        gx[i] = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) d[i * S + k] = gG[i * S + k];
    }
    // reverse sweep over the columns: d = adjoint of L, turned into the adjoint of Sigma column by column
#pragma unroll
    for (int j = S - 1; j >= 0; --j) {
        const float ljj = L[j * S + j], c = floor_nan(ljj);
        float dc = 0.f;
#pragma unroll
        for (int i = j + 1; i < S; ++i) {
            const float dl = d[i * S + j], da = dl / c;   // L_ij = a_ij / c:  d a_ij = dl / c,  d c -= dl L_ij / c
            dc -= da * L[i * S + j];
            d[i * S + j] = da;
#pragma unroll
            for (int k = 0; k < j; ++k) { d[i * S + k] -= da * L[j * S + k]; d[j * S + k] -= da * L[i * S + k]; }
        }
        const float dljj = d[j * S + j] + (ljj >= kEmFloor ? dc : 0.f);
        const float ds = sd[j] >= kEmFloor ? dljj / (2.f * ljj) : 0.f;
        d[j * S + j] = ds;
#pragma unroll
        for (int k = 0; k < j; ++k) d[j * S + k] -= 2.f * ds * L[j * S + k];
    }
    // through Sigma and f to the propensities, then h_j = theta_j prod_i x_i^r_ji.  With KIN the rate-law reactions keep their
    // dh_j for a second loop: one loop with both bodies is too large to unroll fully at S = 8, NR = 16 (its arrays would go to
    // scratch)
    float dhl[KIN ? NR : 1];
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        if (j < n.R) {
            float dh = 0.f;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                float acc = gf[i];
#pragma unroll
                for (int k = 0; k <= i; ++k) acc += d[i * S + k] * n.change[j][k];
                dh += acc * n.change[j][i];
            }
            if constexpr (KIN) {
                dhl[j] = dh;
                if (crn_rl(n.law[j]) != VSDE_CRN_LAW_MASS_ACTION) continue;
            }
            float pre[S], m = 1.f;
#pragma unroll
            for (int i = 0; i < S; ++i) { pre[i] = m; m *= crn_pow(x[i], n.order[j][i]); }
            gth[j] += dh * m;
            const float dm = dh * th[j];
            float suf = 1.f;
#pragma unroll
            for (int i = S - 1; i >= 0; --i) {
                gx[i] += dm * (pre[i] * suf) * crn_dpow(x[i], n.order[j][i]);
                suf *= crn_pow(x[i], n.order[j][i]);
            }
        }
    }
    if constexpr (KIN) {
        // g = num / (c + a), num = a (activation) or c (repression):  dg/du = +-n u^(n-1) c / (c+a)^2,  dg/dK = -+n K^(n-1) a /
        // (c+a)^2; x_s gets dg/du only where x_s >= 0 (torch.clamp's rule)
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            if (j < n.R) {
                const int law = crn_rl(n.law[j]);
                if (law != VSDE_CRN_LAW_MASS_ACTION) {
                    const int s = crn_rl(n.mod[j]), e = crn_rl(n.hill_n[j]);
                    const bool act = law == VSDE_CRN_LAW_HILL_ACTIVATION;
                    const float dh = dhl[j], xs = crn_pick<S>(x, s), u = xs < 0.f ? 0.f : xs, K = th[NR + j];
                    const float a = crn_hpow(u, e), c = crn_hpow(K, e), den = c + a;
                    gth[j] += dh * ((act ? a : c) / den);
                    const float w = dh * th[j] / (den * den), fe = (float)e;
                    const float gu = xs >= 0.f ? w * c * fe * crn_pow(u, e - 1) : 0.f;
                    const float gk = w * a * fe * crn_pow(K, e - 1);
#pragma unroll
                    for (int i = 0; i < S; ++i)
                        if (i == s) gx[i] += act ? gu : -gu;
                    gth[NR + j] += act ? -gk : gk;
                }
            }
        }
    }
}

// y = x + f dt + (G e) sqrt(dt)
template <int S, int NR, bool KIN = false>
__device__ __forceinline__ void crn_em_step(const CrnNet &n, const float *x, const float *th, const float *e, float dt, float sqdt,
                                            float *y) {
    float f[S], G[S * S];
    crn_coef<S, NR, KIN>(n, x, th, f, G);
#pragma unroll
    for (int i = 0; i < S; ++i) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k <= i; ++k) acc += G[i * S + k] * e[k];
        y[i] = x[i] + f[i] * dt + acc * sqdt;
    }
}

// reverse-mode derivative of crn_em_step: a = dL/dy (already masked by the clamp) -> ax = dL/dx, gth += dL/dtheta
template <int S, int NR, bool KIN = false>
__device__ __forceinline__ void crn_em_step_bwd(const CrnNet &n, const float *x, const float *th, const float *e, const float *a,
                                                float dt, float sqdt, float *ax, float *gth) {
    float gf[S], gG[S * S], gx[S];
#pragma unroll
    for (int i = 0; i < S; ++i) {
        gf[i] = a[i] * dt;
#pragma unroll
        for (int k = 0; k <= i; ++k) gG[i * S + k] = a[i] * e[k] * sqdt;
    }
    crn_coef_bwd<S, NR, KIN>(n, x, th, gf, gG, gx, gth);
#pragma unroll
    for (int i = 0; i < S; ++i) ax[i] = a[i] + gx[i];
}

// the effective constants of path b, rates [B][2R] = (k_0 .. k_{R-1}, K_0 .. K_{R-1}), into th [2 NR] at compile-time
// register offsets: th[j] = k_j, th[NR + j] = K_j (R at run time, the rest 1), and the gradient gth [2 NR] back into g [B][2R]
template <int NR>
__device__ __forceinline__ void crn_load_rates(float *th, const float *rates, int b, int R, bool valid) {
    const float *r = rates + (int64_t)b * 2 * R;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        th[j] = (valid && j < R) ? r[j] : 1.f;
        th[NR + j] = (valid && j < R) ? r[R + j] : 1.f;
    }
}
template <int NR> __device__ __forceinline__ void crn_store_rates(float *g, const float *gth, int b, int R) {
    float *o = g + (int64_t)b * 2 * R;
#pragma unroll
    for (int j = 0; j < NR; ++j)
        if (j < R) { o[j] = gth[j]; o[R + j] = gth[NR + j]; }
}

// ---------------------------------------------------------------------------------------------------------------------
// Host: the model route of an entry point and its compile-time dispatch, shared by the simulator (vsde_sde.hip), the log-weight
// (vsde_elbo.hip) and the particle-filter (vsde_filter.hip) entry points.  A route is a built-in kind 1..3 the caller names, or
// kind 4: a reaction network (vsde_crn_*), with rate laws for the vsde_crn_kinetic_* entry points (theta is then the effective
// constants [2R]).  `descriptors` counts what the entry point takes, so a NULL pointer is an error and not another route.
struct SdeRoute {
    int kind;
    int descriptors = 0;   // 0: built-in kind; 1: network; 2: network and rate laws
    const vsde_crn_network *net = nullptr;
    const vsde_crn_kinetics *kin = nullptr;
};
static inline SdeRoute crn_route(const vsde_crn_network *net) { return {4, 1, net, nullptr}; }
static inline SdeRoute crn_route(const vsde_crn_network *net, const vsde_crn_kinetics *kin) { return {4, 2, net, kin}; }

// the built-in kinds' relations between S and P
static inline int kind_check(int kind, int S, int P) {
    VSDE_CHECK_ARG(kind >= 1 && kind <= 3, VSDE_E_BADARG, "unknown built-in SDE kind %d", kind);
    VSDE_CHECK_ARG(kind != 1 || (S == 1 && P == 3), VSDE_E_BADARG, "Ornstein-Uhlenbeck needs state_dim 1, sde_param_dim 3");
    VSDE_CHECK_ARG(kind != 2 || (S == 2 && P == 3), VSDE_E_BADARG, "Lotka-Volterra needs state_dim 2, sde_param_dim 3");
    VSDE_CHECK_ARG(kind != 3 || P == 2 * S, VSDE_E_BADARG, "linear-diagonal SDE needs sde_param_dim = 2 state_dim");
    return 0;
}

// the descriptors of a kind-4 route against the call's S / P, converted into n
static inline int crn_route_net(const SdeRoute &rt, int S, int P, CrnNet &n) {
    const int rc = crn_net(rt.net, S, P, n, rt.descriptors == 2);
    return rc || rt.descriptors < 2 ? rc : crn_kinetics(rt.kin, S, n);
}

// the route's own argument checks
static inline int route_check(const SdeRoute &rt, int S, int P, CrnNet &n) {
    return rt.descriptors ? crn_route_net(rt, S, P, n) : kind_check(rt.kind, S, P);
}

template <int V> using IntC = std::integral_constant<int, V>;

// f(IntC<n>) for the run-time n in 1..MAX (the callers' argument checks keep n in range)
template <int MAX, int N = 1, class F> static int dispatch_dim(int n, F &&f) {
    if (n == N) return f(IntC<N>{});
    if constexpr (N < MAX) {
        return dispatch_dim<MAX, N + 1>(n, f);
    } else {
        set_error("state_dim %d not supported (1..%d)", n, MAX);
        return VSDE_E_STATE;
    }
}

// f(IntC<S>, IntC<NR>) for the run-time S in 1..MAX_S and the reaction bound NR of R
template <int MAX_S = kCrnMaxS, class F> static int crn_dispatch(int S, int R, F &&f) {
    return dispatch_dim<MAX_S>(S, [&](auto ns) {
        if (R <= 4) return f(ns, IntC<4>{});
        if (R <= 8) return f(ns, IntC<8>{});
        return f(ns, IntC<kCrnMaxR>{});
    });
}

// f(IntC<KIND>, IntC<NS>, IntC<NR>, std::bool_constant<KIN>): the template arguments of the route's kernels (R: the network's
// reaction count).  Kind 3 is dispatched on S in 1..DIAG_MAX_S, or, with DIAG_MAX_S = 0 (kernels that read S at run time), called
// once with EmDims<3>; kind 4 on S in 1..CRN_MAX_S.
template <int DIAG_MAX_S, int CRN_MAX_S = kCrnMaxS, class F> static int route_dispatch(const SdeRoute &rt, int S, int R, F &&f) {
    constexpr std::false_type no{};
    switch (rt.kind) {
        case 1: return f(IntC<1>{}, IntC<EmDims<1>::S>{}, IntC<EmDims<1>::P>{}, no);
        case 2: return f(IntC<2>{}, IntC<EmDims<2>::S>{}, IntC<EmDims<2>::P>{}, no);
        case 3:
            if constexpr (DIAG_MAX_S == 0) return f(IntC<3>{}, IntC<EmDims<3>::S>{}, IntC<EmDims<3>::P>{}, no);
            else return dispatch_dim<DIAG_MAX_S>(S, [&](auto ns) { return f(IntC<3>{}, ns, IntC<EmDims<3>::P>{}, no); });
        default:
            if (rt.descriptors == 2) return crn_dispatch<CRN_MAX_S>(S, R, [&](auto ns, auto nr) { return f(IntC<4>{}, ns, nr, std::true_type{}); });
            return crn_dispatch<CRN_MAX_S>(S, R, [&](auto ns, auto nr) { return f(IntC<4>{}, ns, nr, no); });
    }
}

}  // namespace vsde
