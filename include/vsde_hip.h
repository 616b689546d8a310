/*
 * vsde_hip.h -- C ABI of libvsde_hip.so, the MI355X (gfx950) implementation of the
 * variational-SDE hot path.  Plain pointers and sizes only; every pointer is a DEVICE
 * pointer unless stated otherwise; `stream` is a hipStream_t passed as void*.
 *
 * Each entry point replaces one interface of the reference (Tom-Ryder/VIforSDEs):
 *
 *   vsde_head_forward        launch_fwd + sde_fwd_kernel   src/variational_sde/kernels/forward.py:378-563
 *                            (called from _SDEFunction.forward, kernels/autograd.py:79-87, and from
 *                             kernels.autograd.sample_diffusion_paths, autograd.py:244-268)
 *   vsde_head_backward       launch_bwd + sde_bwd_kernel   src/variational_sde/kernels/backward.py:627-784
 *                            (called from _SDEFunction.backward, kernels/autograd.py:191-201)
 *   vsde_elbo_path_terms     the B*T-sized part of compute_evidence_lower_bound
 *   vsde_elbo_path_terms_bwd   src/variational_sde/inference/evidence_lower_bound.py:42-50,77-83 and
 *                              DiffusionPathSample.log_jacobian, inference/types.py:23-24
 *
 * Weight tensors use torch.nn.GRU's native layout exactly as they are handed to
 * _SDEFunction.apply (kernels/autograd.py:46-56): W_ih_l0[3H][S+C+P] with input order
 * [state | context | theta] (models/head.py:75), W_hh_l0[3H][H], biases [3H], the stacked
 * layers >=1 as [L-1][3H][H] / [L-1][3H], out_weight[S+ntril][H], out_bias[S+ntril];
 * gate order r, z(u), n.  Gradients come back in the same layout and the same order as
 * launch_bwd's 13-tuple (backward.py:766-784).
 *
 * Error convention: every function returns 0 on success, a negative VSDE_E_* code for
 * argument errors (the Python host maps them to ValueError like the reference's own checks,
 * models/head.py:33-36) or a positive hipError_t.  vsde_last_error() returns a static,
 * thread-local, human-readable message for the last failure.
 *
 * Threading/streams: functions only enqueue work on `stream` (no device synchronisation, no
 * allocation); all scratch memory is the caller-provided workspace, sized by the matching
 * *_workspace_bytes query.  Inputs are never written; outputs are fully overwritten.
 */
#ifndef VSDE_HIP_H
#define VSDE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VSDE_ABI_VERSION 1

#define VSDE_E_BADARG (-1)   /* shape/pointer/dtype argument invalid                    */
#define VSDE_E_LAYERS (-2)   /* num_layers outside [1, 4]  (kernels/constants.py:13)    */
#define VSDE_E_HIDDEN (-3)   /* hidden_dim not supported by the compiled kernels        */
#define VSDE_E_WORKSPACE (-4) /* workspace too small                                    */
#define VSDE_E_STATE (-5)    /* state_dim not supported by the compiled kernels         */

#define VSDE_MAX_LAYERS 4
#define VSDE_MAX_HIDDEN 1024 /* tuned kernels: hidden_dim <= 64; generic kernels: one thread per unit up to 1024 */
#define VSDE_MAX_STATE 32    /* tuned kernels: S + S(S+1)/2 <= 64 emission rows (S <= 9); generic kernels beyond */

#define VSDE_CTX_F32 0
#define VSDE_CTX_BF16 1

int vsde_abi_version(void);
/* 1: this library was built with -DVSDE_ABLATIONS (A/B switches read from the environment, losing kernel variants compiled in:
   tools and their tests only); 0: the shipped library. */
int vsde_build_ablations(void);
const char *vsde_last_error(void);

/* Problem dimensions shared by the head entry points (names as in SURVEY.md section 8). */
typedef struct vsde_head_dims {
    int B; /* Monte-Carlo sample paths in this launch          */
    int T; /* Euler-Maruyama steps (= context.shape[1])        */
    int S; /* state_dim                                        */
    int P; /* sde_param_dim                                    */
    int C; /* context_dim (= encoder hidden_dim)               */
    int H; /* GRU hidden_dim                                   */
    int L; /* GRU num_layers                                   */
} vsde_head_dims;

/* The ten weight tensors of the head (device pointers, fp32, contiguous). */
typedef struct vsde_head_weights {
    const float *W_ih_l0, *W_hh_l0, *b_ih_l0, *b_hh_l0;
    const float *W_ih_stack, *W_hh_stack, *b_ih_stack, *b_hh_stack; /* may be NULL when L == 1 */
    const float *out_weight, *out_bias;
} vsde_head_weights;

/* Strided view of the encoder context: element (b, t, c) lives at
 * base + (b*batch_stride + t*step_stride + c) * sizeof(elem).  This lets the caller pass the
 * reference's non-contiguous context[:, :-1] slice (inference/diffusion_path_sampler.py:61)
 * and the autocast bf16 context without the .contiguous().float() copies of forward.py:495. */
typedef struct vsde_context_view {
    const void *base;
    int dtype; /* VSDE_CTX_F32 or VSDE_CTX_BF16 */
    int64_t batch_stride;
    int64_t step_stride;
} vsde_context_view;

size_t vsde_head_forward_workspace_bytes(const vsde_head_dims *d);

/* Fused multi-layer-GRU + Gaussian emission + Euler-Maruyama time stepping.
 *   x0[B][S], theta[B][P], eps[B][T][S]
 *   paths[B][T+1][S], means[B][T][S], chol[B][T][S][S] (strict upper triangle written as 0)
 * Training mode (save != 0) additionally fills what the backward needs
 * (kernels/weights.py:11-23 SavedActivations), packed as
 *   chol_raw[B][T][ntril]  and  acts[B][T][L][5][H] with slots (h, r, z, n, n_hh). */
int vsde_head_forward(const vsde_head_dims *d, const float *x0, const vsde_context_view *ctx,
                      const float *theta, const float *eps, const vsde_head_weights *w,
                      double time_step, double diag_min, int save,
                      float *paths, float *means, float *chol, float *chol_raw, float *acts,
                      void *workspace, size_t workspace_bytes, void *stream);

/* The 13 gradient outputs of launch_bwd, same order (backward.py:766-784). */
typedef struct vsde_head_grads {
    float *x0;          /* [B][S]        */
    float *context;     /* [B][T][C]     */
    float *theta;       /* [B][P]        */
    float *W_ih_l0, *W_hh_l0, *b_ih_l0, *b_hh_l0;
    float *W_ih_stack, *W_hh_stack, *b_ih_stack, *b_hh_stack; /* unused when L == 1 */
    float *out_weight, *out_bias;
    /* placement of the context gradient (0, 0 = fp32 [B][T][C] contiguous): dtype 1 writes bf16 through the same pointer;
     * a batch stride (elements, >= T*C) lets it be the leading T rows of every slab of a [B][T+1][C] buffer, i.e. the
     * gradient of the encoder output itself, whose last token the head never reads (diffusion_path_sampler.py:66). */
    int context_dtype;
    int64_t context_batch_stride;
} vsde_head_grads;

size_t vsde_head_backward_workspace_bytes(const vsde_head_dims *d);

/* Reverse-time BPTT through the fused head.  g_paths[B][T+1][S], g_means[B][T][S],
 * g_chol[B][T][S][S] are the upstream gradients; paths/chol_raw/acts are the tensors the
 * forward saved.  Deterministic: weight gradients are tree-reduced, no atomics
 * (the reference uses global fp32 atomics, backward.py:108-139,575-590). */
int vsde_head_backward(const vsde_head_dims *d, const float *g_paths, const float *g_means,
                       const float *g_chol, const vsde_context_view *ctx, const float *theta,
                       const float *eps, const float *paths, const float *chol_raw,
                       const float *acts, const vsde_head_weights *w, double time_step,
                       double diag_min, const vsde_head_grads *grads, void *workspace,
                       size_t workspace_bytes, void *stream);

/* Per-sample path terms of the ELBO.  z, x: [B][T+1][S] (x = StateSpace.to_state(z));
 * means/drift: [B][T][S]; chol/diffusion: [B][T][S][S] lower-triangular factors;
 * positive_mask: S bytes on the HOST (state_space.positive_dims).
 * Outputs [B]: sde_lp, gen_lp, log_jac. */
int vsde_elbo_path_terms(int B, int T, int S, const float *z, const float *x, const float *means,
                         const float *chol, const float *drift, const float *diffusion,
                         const uint8_t *positive_mask_host, double time_step,
                         float *sde_lp, float *gen_lp, float *log_jac, void *stream);

/* Adjoint of vsde_elbo_path_terms for upstream per-sample gradients g_sde/g_gen/g_jac [B].
 * Outputs are fully overwritten: g_z, g_x [B][T+1][S]; g_means, g_drift [B][T][S];
 * g_chol, g_diffusion [B][T][S][S].  B <= 65535 (one grid row per path): a larger batch is an argument error
 * before any launch -- split it over several calls. */
int vsde_elbo_path_terms_bwd(int B, int T, int S, const float *z, const float *x,
                             const float *means, const float *chol, const float *drift,
                             const float *diffusion, const uint8_t *positive_mask_host,
                             double time_step, const float *g_sde, const float *g_gen,
                             const float *g_jac, float *g_z, float *g_x, float *g_means,
                             float *g_chol, float *g_drift, float *g_diffusion, void *stream);

/* ---- Fused encoder operators (SiT blocks of the observation encoder) -------------------------
 * dtype: 0 = f32, 1 = bf16 for every `void *` tensor of the call; cos/sin tables, RMS weights,
 * lambda, mean/rstd are always f32.  Contiguous tensors; B = batch rows, N = tokens per row.
 * Replaces the unfused torch chains of primitives/sit.py:99-128 (LayerNorm -> (1+scale)x+shift,
 * gate*branch residual), primitives/attn.py:80-113 (QK RMS-norm, RoPE, value-residual mix, head
 * layout, sigmoid output gate) and primitives/mlp.py:21-24 (SwiGLU activation). */
/* mod_pitch: row pitch (elements) of the per-batch-row vectors scale / shift / gate AND of their gradient outputs; 0 = C
 * (contiguous [B][C]).  A pitch > C lets all of them be column ranges of one [B][pitch] buffer -- the output of the single
 * GEMM that produces every block's adaLN parameters, and its gradient -- with no copies in either direction. */
int vsde_ln_modulate_fwd(int dtype, const void *x, const void *scale, const void *shift, void *y, float *mean,
                         float *rstd, int64_t B, int N, int C, double eps, int64_t mod_pitch, void *stream);
/* The two backward passes below also produce per-(batch row, channel) sums over the tokens (dscale/dshift, dgate);
 * they need vsde_colsum_workspace_bytes(B, C) bytes of device scratch for the fp32 partials. */
size_t vsde_colsum_workspace_bytes(int64_t B, int C);
/* dres (optional, [B][N][C]) is added to dx: the gradient reaching x through the residual branch */
int vsde_ln_modulate_bwd(int dtype, const void *x, const void *scale, const void *dy, const float *mean,
                         const float *rstd, const void *dres, void *dx, void *dscale, void *dshift, int64_t B, int N, int C,
                         int64_t mod_pitch, void *workspace, size_t workspace_bytes, void *stream);
/* Gated residual fused with the LayerNorm-modulate that follows it (primitives/sit.py:73-79 + next norm):
 *   xnew = x + gate*y;  h = LN(xnew)*(1+scale) + shift.   Backward: dxnew (optional) is the gradient reaching xnew from its
 *   other consumers; dx = dxnew + LNbwd(dh) is the gradient of x, dy = gate*dx, dgate/dscale/dshift are token sums. */
int vsde_residual_ln_fwd(int dtype, const void *x, const void *y, const void *gate, const void *scale, const void *shift,
                         void *xnew, void *h, float *mean, float *rstd, int64_t B, int N, int C, double eps, int64_t mod_pitch,
                         void *stream);
int vsde_residual_ln_bwd(int dtype, const void *xnew, const void *y, const void *gate, const void *scale, const void *dh,
                         const void *dxnew, const float *mean, const float *rstd, void *dx, void *dy, void *dgate,
                         void *dscale, void *dshift, int64_t B, int N, int C, int64_t mod_pitch, void *workspace,
                         size_t workspace_bytes, void *stream);
int vsde_gated_residual_fwd(int dtype, const void *x, const void *y, const void *gate, void *out, int64_t B, int N, int C,
                            int64_t mod_pitch, void *stream);
int vsde_gated_residual_bwd(int dtype, const void *y, const void *gate, const void *dout, void *dy, void *dgate, int64_t B,
                            int N, int C, int64_t mod_pitch, void *workspace, size_t workspace_bytes, void *stream);
/* gated_residual_bwd: C % 4 == 0 and at most 256 lanes of 16 (bf16: 8 or 16) bytes per token -- C <= 1024 in f32, in bf16
 * C <= 2048 when C % 8 == 0 and C <= 1024 otherwise; wider rows return VSDE_E_BADARG. */
int vsde_swiglu_fwd(int dtype, const void *u, void *out, int64_t M, int H2, void *stream);
int vsde_swiglu_bwd(int dtype, const void *u, const void *dout, void *du, int64_t M, int H2, void *stream);
/* token_major selects the memory layout of the per-head tensors (attn, dattn, q, k, v, v0, dq, dk, dv, dv0):
 * 0 = [B][heads][N][d] (the reference's layout after attn.py:96), 1 = [B][N][heads][d] (what the memory-efficient
 * SDPA kernels read and write natively, so no transposing copies are needed around the attention call). */
int vsde_gate_merge_fwd(int dtype, const void *attn, const void *glog, void *out, int64_t B, int N, int heads, int d,
                        int token_major, int64_t glog_stride, void *stream);
int vsde_gate_merge_bwd(int dtype, const void *attn, const void *glog, const void *dout, void *dattn, void *dglog, int64_t B,
                        int N, int heads, int d, int token_major, int64_t glog_stride, void *stream);
/* qkv[B][N][3C] -> q, k, v; cosT/sinT [N][d/2]; wq/wk [d]; v0 optional, same layout as v.
 * row_stride (>= 3C elements) / glog_stride (>= d) are the row pitches of qkv+dqkv / glog+dglog, so both can be column
 * ranges of the output of ONE merged [qkv | gate] projection (and of its gradient buffer). */
int vsde_qk_norm_rope_fwd(int dtype, const void *qkv, const float *cosT, const float *sinT, const float *wq, const float *wk,
                          const void *v0, const float *lam, void *q, void *k, void *v, int64_t B, int N, int heads, int d,
                          double eps, int token_major, int64_t row_stride, void *stream);
int64_t vsde_qk_norm_rope_bwd_partials(int64_t B, int N, int heads, int d);
int vsde_qk_norm_rope_bwd(int dtype, const void *qkv, const float *cosT, const float *sinT, const float *wq, const float *wk,
                          const void *v0, const float *lam, const void *dq, const void *dk, const void *dv, void *dqkv,
                          void *dv0, float *dlam_partial, int64_t B, int N, int heads, int d, double eps, int token_major,
                          int64_t row_stride, int dv0_accumulate, const void *dv_extra, void *stream);
/* dv0_accumulate != 0: dv0 += (1-lam) dv (all blocks' value-residual gradients collect in one buffer); dv_extra (optional,
 * layout of dv) is added to dv first -- the block that produced v0 gets that buffer next to its own attention's dv. */

/* Attention core (bf16, head_dim 64 or 128).  head_dim 64 with N <= vsde_attention_max_tokens() runs the kernels that keep K
 * and V of one (batch, head) resident in LDS (the encoder's shape class at the OU / LV grids); longer sequences and head_dim
 * 128 (the 1001-token, 512 / 4-head stress configuration) run the kernels that stream 32-token tiles through LDS:  o = softmax(scale * q k^T) v  with q, k, v, o token-major [B][N][H][64];
 * lse [B][H][N] = natural-log sum-exp of the scaled scores (what a flash-attention backward consumes).
 * Replaces F.scaled_dot_product_attention at primitives/attn.py:104-106 for these shapes. */
int vsde_attention_max_tokens(void);
int vsde_attention_fwd_bf16(const void *q, const void *k, const void *v, void *o, float *lse, int64_t B, int N, int H,
                            int head_dim, double scale, void *stream);
/* Backward of the above (same limits): dq, dk, dv token-major bf16 from dout, q, k, v, o and the forward's lse;
 * delta [B][H][N] fp32 is scratch (row sums <dout, o>).  Deterministic (no atomics). */
int vsde_attention_bwd_bf16(const void *dout, const void *q, const void *k, const void *v, const void *o, const float *lse,
                            void *dq, void *dk, void *dv, float *delta, int64_t B, int N, int H, int head_dim, double scale,
                            void *stream);

/* ---- Training step with the projection-side elementwise work folded into the attention kernels ------------------------
 * (primitives/attn.py:80-113 between the [q | k | v | gate] projection and the output projection; head_dim 64 and
 * N <= vsde_attention_max_tokens(): vsde_attention_fused_supported != 0.)  The forward is vsde_linear_qknorm_bf16 (with its
 * rinv / vdiff outputs) + vsde_attention_fwd_gated_bf16; the backward is vsde_gate_bwd_delta + vsde_attention_bwd_fused_bf16,
 * which leaves the gradient dy [M][ldy] of the projection output ready for its input- and weight-gradient GEMMs.  Replaces
 * the separate qk_norm_rope fwd / bwd and gate_merge fwd passes of the unfused training chain.
 *   vsde_attention_fwd_gated_bf16   o[b,n,h,:] = softmax(..) v * s[b n][0..64), s = rnd(sigmoid(gate logit)) as written by
 *                                   vsde_linear_qknorm_bf16(gate_sigmoid = 1)          (the merged [B,N,(h d)] rows)
 *   vsde_gate_bwd_delta             dattn = dout * s, dgate[m][0..64) = (1 - s) sum_h dout * og (the gradient of the LOGITS),
 *                                   delta[b,h,n] = <dout, og>
 *   vsde_attention_bwd_fused_bf16   dattn, the forward's q, k, v, lse and that delta -> dy columns [dq_raw | dk_raw | dv_raw]:
 *       the RoPE / RMS-norm backward from the saved rotated rows and rinv [M][2H] (weights wq / wk all non-zero), the value mix
 *       from vdiff = v_raw - v0 (NULL: no mixing): dv_raw = lam dv, dv0 (+)= (1 - lam) dv, dlam_partial[B H ceil(N/32)] partial
 *       sums of <dv, vdiff> (vsde_attention_bwd_fused_partials entries); dv_extra (NULL or [M][64H]) is added to dv first. */
int vsde_attention_fused_supported(int N, int head_dim);
int vsde_attention_fwd_gated_bf16(const void *q, const void *k, const void *v, const void *gate, int64_t ldg, void *o, float *lse,
                                  int64_t B, int N, int H, double scale, void *stream);
int vsde_gate_bwd_delta(const void *dout, const void *og, const void *gate, int64_t ldg, void *dattn, void *dgate, int64_t ldd,
                        float *delta, int64_t B, int N, int H, void *stream);
int64_t vsde_attention_bwd_fused_partials(int64_t B, int N, int H);
int vsde_attention_bwd_fused_bf16(const void *dattn, const void *q, const void *k, const void *v, const float *lse, const float *delta,
                                  const float *rinv, const float *cosT, const float *sinT, const float *wq, const float *wk,
                                  const void *vdiff, const float *lam, void *dv0, int dv0_accumulate, const void *dv_extra, void *dy,
                                  int64_t ldy, float *dlam_partial, int64_t B, int N, int H, double scale, void *stream);

/* Weight and bias gradient of y = x W^T + b for bf16 activations:  dW[N][K] = dy^T x,  db[N] = colsum(dy)
 * (db may be NULL).  dy [M][N], x [M][K] bf16 contiguous, N % 8 == K % 8 == 0; results fp32, deterministic.
 * Replaces torch's hipBLASLt "wgrad" GEMM + bf16 column-sum kernel of every encoder nn.Linear
 * (reference: primitives/attn.py:46-47,54, primitives/mlp.py:41-44 via torch autograd). */
size_t vsde_linear_wgrad_workspace_bytes(int64_t M, int N, int K);
int vsde_linear_wgrad_bf16(const void *dy, const void *x, int64_t M, int N, int K, float *dW, float *db, void *workspace,
                           size_t workspace_bytes, void *stream);
/* Same, with the rows of the product scattered: row n of dY^T X (and of the column sums) is stored at dW[row_map[n]] /
 * db[row_map[n]] (int32 [N] on the device; negative = dropped).  Lets a weight packed in a permuted / padded row order (the
 * 16-row-interleaved SwiGLU input projection) hand its gradient back in the parameter's own row order without a gather. */
int vsde_linear_wgrad_bf16_rows(const void *dy, const void *x, int64_t M, int N, int K, float *dW, float *db,
                                const int32_t *row_map, void *workspace, size_t workspace_bytes, void *stream);
/* Several weight gradients in (at most) two launches per tile width plus their reductions instead of one pair per problem:
 * item i is exactly one vsde_linear_wgrad_bf16_rows call (with group_plan = 0: same plan, same fixed-order sums, bit-identical).  At a few
 * thousand rows every such problem is a ~20 us kernel that cannot fill the chip alone (the OU example: 25 per optimizer step);
 * the trainer collects the encoder's weight gradients of one backward pass and issues them together. */
typedef struct VsdeWgradItem {
    const void *dy, *x;      /* bf16 [M][N], [M][K], contiguous, 16-byte aligned */
    int64_t M;
    int32_t N, K;            /* multiples of 8 */
    float *dW, *db;          /* fp32 [rows][K], [rows]; db may be NULL */
    const int32_t *row_map;  /* device int32 [N] or NULL (identity) */
} VsdeWgradItem;
size_t vsde_linear_wgrad_group_workspace_bytes(int n, const void *items /* VsdeWgradItem[n], host */);
/* group_plan != 0: split counts chosen for the group as a whole (fewer, longer workgroups per problem: less partial-tile traffic);
 * the fixed-order sums then differ in order from a single launch's -- deterministic, but not bit-identical to it. */
int vsde_linear_wgrad_group_bf16(int n, const void *items, int group_plan, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Dense contractions of the encoder on bf16 MFMA ----------------------------------------------------------------
 * y[M][N] = x[M][K] w[N][K]^T + bias[N]   (x, w, bias, y bf16; fp32 accumulation).  Replaces the hipBLASLt GEMMs behind
 * nn.Linear in primitives/attn.py:46-47,54,113 (qkv / gate / out projections), primitives/mlp.py:41-54 (SwiGLU pair) and
 * primitives/sit.py:186 (output projection), and -- called with the transposed weight -- their input gradients.
 * ldx / ldy: row pitches in elements (multiples of 8; 16-byte aligned bases).  epilogue:
 *   VSDE_EPI_PLAIN        y = acc + bias
 *   VSDE_EPI_SWIGLU       w packs the SwiGLU input projection with its two halves interleaved in blocks of 16 rows
 *                         ([a_0..15 | b_0..15 | a_16..31 | ...]); u = acc + bias goes to y (may be NULL when the caller
 *                         does not need it), s_out[M][N/2] = silu(a) * b  (mlp.py:21-24)
 *   VSDE_EPI_SWIGLU_BWD   acc is ds (gradient of s, N = width of s); u_in[M][2N] is the saved interleaved u and
 *                         y[M][2N] receives du = (da | db) in the same interleaved layout
 * vsde_linear_bf16_supported returns 0 when the shape is outside the compiled kernels (K in {128, 256} with N % 64 == 0;
 * for the plain epilogue also any K % 64 == 0 with N % 128 == 0); callers then keep their library GEMM. */
#define VSDE_EPI_PLAIN 0
#define VSDE_EPI_SWIGLU 1
#define VSDE_EPI_SWIGLU_BWD 2
int vsde_linear_bf16_supported(int64_t M, int N, int K, int epilogue);
int vsde_linear_bf16(const void *x, int64_t ldx, const void *w, const void *bias, void *y, int64_t ldy, int64_t M, int N, int K,
                     int epilogue, void *s_out, int64_t lds, const void *u_in, int64_t ldu, void *stream);
/* Attention projection (primitives/attn.py:80-103 in one kernel): y = x W^T + b with W = [q | k | v | gate] rows
 * (N = 3 heads*64 + gate_width, K in {128, 256}), and in the epilogue RMS-norm (weights wq / wk [64], eps) + RoPE (cos / sin tables
 * [tokens][32], row m is token m % tokens, rotary pairs (i, i + 32)) on every q / k head, v = lam v + (1 - lam) v0 when residual
 * values are given, everything written straight in the attention layout: q, k, v [M][heads*64] (token-major [B,N,h,64]),
 * gate logits [M][ldg].  Same rounding points as vsde_linear_bf16 followed by vsde_qk_norm_rope_fwd.  For the training step
 * (both may be NULL): rinv [M][2 heads] fp32 receives the inverse RMS of every q / k head row and vdiff [M][heads*64] bf16
 * v_raw - v0 -- all the backward needs, the raw projection is never written; gate_sigmoid != 0: the gate block is written as
 * rnd(sigmoid(logit)), the factor vsde_attention_fwd_gated_bf16 multiplies by (one sigmoid per token and channel, not per head). */
int vsde_linear_qknorm_bf16(const void *x, int64_t ldx, const void *w, const void *bias, int64_t M, int K, int heads, int gate_width,
                            int tokens, const float *cosT, const float *sinT, const float *wq, const float *wk, const void *v0,
                            const float *lam, double eps, void *q, void *k, void *v, void *gate, int64_t ldg, int gate_sigmoid,
                            float *rinv, void *vdiff, void *stream);
/* No-grad attention output projection with gate_merge folded into the operand load (primitives/attn.py:107-110):
 * y = (attn * sigmoid(gate[:, k % 64])) W^T + b for attn [M][K] (token-major heads of 64), gate logits [M][ldgate].
 * Rows kernel shapes only (K in {128, 256}, N % 64 == 0). */
int vsde_linear_gated_bf16(const void *attn, int64_t ldx, const void *gate, int64_t ldgate, const void *w, const void *bias, void *y,
                           int64_t ldy, int64_t M, int N, int K, void *stream);

/* Training step: input gradient of the attention output projection with the backward of the sigmoid output gate in its
 * epilogue (primitives/attn.py:107-113; replaces vsde_linear_bf16 on the transposed weight followed by vsde_gate_bwd_delta):
 * d = dy w_t^T is the gradient of the merged rows [M][heads*64] (w_t [heads*64][K] = the projection weight transposed; K in
 * {128, 256}); with og (the merged gated rows) and the gate factors s [M][lds] it leaves as
 *   dattn = d * s,   delta[b,h,n] = <d, og>,   dgate[m][0..64) = (1 - s) sum_h d og   (gradient of the gate LOGITS, row pitch ldd)
 * -- d itself is never written.  Rows are (batch, token) pairs, m = b * tokens + n. */
int vsde_linear_gate_bwd_bf16(const void *dy, int64_t ldy, const void *w_t, const void *og, const void *s, int64_t lds, void *dattn,
                              void *dgate, int64_t ldd, float *delta, int64_t M, int K, int heads, int tokens, void *stream);

/* ---- The SwiGLU feed-forward of a SiT block as one kernel per direction (csrc/vsde_mlp.hip, round 5) -------------------------
 * Replaces primitives/mlp.py:50-54 under autocast:  y = W_out (silu(a) * b) + b_out,  [a | b] = W_in x + b_in,  x [M][C] bf16,
 * hidden size H (a multiple of 64, zero-padded), C in {128, 256}.  The weights are handed over as tile IMAGES (T = H / 16 tiles;
 * sizes per tile from vsde_mlp_image_bytes; layouts in csrc/vsde_mlp.hip, built by primitives/fused.py::MlpImages):
 *   w1_img [T][32 rows][C + 8] bf16 (+ padding to whole KB): row 8 g + 4 h + i of tile t = (g < 2 ? a : b) unit 16 t + 8 h + 4 (g & 1) + i
 *   w2_img [T][2][C][8] bf16: W_out[n][16 t + 8 h + 0..7];   b1_img [T][64] fp32: b_in in w1_img's row order (32 used)
 * s_out (training only, else NULL): silu(a) * b [M][lds] bf16 in natural unit order, what the weight gradient of W_out needs; the
 * pre-activations are never written (the backward recomputes them). */
/* Block form (no-grad sampling): the gated residuals and modulated LayerNorms on either side of the MLP are the kernel's prologue
 * and epilogue (reference primitives/sit.py:112-128 under autocast, bf16 roundings where the unfused chain has them):
 *   x1 = x + ga * yin;  tok = x1 + gm * mlp(LN(x1) (1 + sc) + sh);  hnext = LN(tok) (1 + sn) + hs   (sn / hs / hnext NULL: last block)
 * x, yin, tok, hnext [M][C] bf16 contiguous; ga .. hs per-batch-row vectors [B][mp] bf16, batch row of row m = m / tokens. */
int vsde_mlp_block_fwd_bf16(const void *x, const void *yin, const void *ga, const void *sc, const void *sh, const void *gm,
                            const void *sn, const void *hs, int64_t mp, int tokens, double eps, double eps_next, const void *w1_img,
                            const void *w2_img, const float *b1_img, const void *b2, void *tok, void *hnext, int64_t M, int C, int H,
                            void *stream);
/* Block form with the attention branch's out projection as the prologue's first product (reference primitives/attn.py:107-110 +
 * sit.py:112-128):  yin = (attn * sigmoid(glog[:, k % 64])) W_o^T + b_o, then as vsde_mlp_block_fwd_bf16.  attn [M][C] bf16 (merged
 * heads, token-major), glog [M][ldg] bf16 (64 gate logits per row), wo_img = W_o as C / 16 tiles in w2_img's format, bo [C] bf16 or
 * NULL.  tok doubles as the scratch that holds x1 between the prologue and the epilogue: it must not alias x. */
int vsde_mlp_attn_block_fwd_bf16(const void *x, const void *attn, const void *glog, int64_t ldg, const void *wo_img, const void *bo,
                                 const void *ga, const void *sc, const void *sh, const void *gm, const void *sn, const void *hs,
                                 int64_t mp, int tokens, double eps, double eps_next, const void *w1_img, const void *w2_img,
                                 const float *b1_img, const void *b2, void *tok, void *hnext, int64_t M, int C, int H, void *stream);
/* y [M][256] = x [M][K] W^T (+ bias) for a DEEP reduction (K % 64 == 0, K >= 256) at the encoder's width 256 (csrc/vsde_mlp.hip,
 * round 5): the SwiGLU output projection (primitives/mlp.py:54) and the input-gradient GEMMs of mlp.py:50 / attn.py:80-82 -- the
 * three products the library ran until then.  w_img = W as K / 16 k-step images [2][256][8] bf16 (W[n][16 t + 8 h + 0..7]: the
 * layout of w2_img above; built by primitives/fused.py::DeepImage), bias [256] bf16 or NULL. */
int vsde_linear_deep256_bf16(const void *x, int64_t ldx, const void *w_img, const void *bias, void *y, int64_t ldy, int64_t M, int K,
                             void *stream);
/* Backward of the SwiGLU MLP in one pass (training step): du [M][2 H] = swiglu'(u) * (dy W_out) and dx [M][C] = du W_in, with the saved
 * pre-activations u and du in the 16-row interleaved layout of primitives/fused.py::swiglu_packs(interleave=True) (64 columns per 32
 * hidden units: [a16 | b16 | a16 | b16]).  img: H / 32 pair-tile images of vsde_mlp_bwd_image_bytes(C) bytes each (layout in
 * csrc/vsde_mlp.hip, built by primitives/fused.py::MlpBwdImages).  Replaces vsde_linear_bf16(EPI_SWIGLU_BWD) + the dx GEMM over du. */
int64_t vsde_mlp_bwd_image_bytes(int C);
int vsde_mlp_bwd_bf16(const void *dy, int64_t lddy, const void *u, int64_t ldu, const void *img, void *du, int64_t lddu, void *dx,
                      int64_t lddx, int64_t M, int C, int H, void *stream);
/* debugging aid (VSDE_MLP_DEBUG=16): device buffer that receives workgroup 0's per-phase cycle stamps */
int vsde_mlp_debug_trace(void *buf);
/* The same for the weight-gradient kernel (eight-wave TN = 256 form): [8 waves][4 phase cycle sums + step count] (tools/wgrad_trace.py). */
int vsde_wgrad_debug_trace(void *buf);
/* ... and for the persistent LDS-resident attention forward: [12 waves][4 phase cycle sums + pair count] (tools/attn_trace.py). */
int vsde_attn_debug_trace(void *buf);
int vsde_mlp_image_bytes(int C, int64_t *w1_tile, int64_t *w2_tile, int64_t *b1_tile);
int vsde_mlp_fwd_bf16(const void *x, int64_t ldx, const void *w1_img, const void *w2_img, const float *b1_img, const void *b2, void *y,
                      int64_t ldy, void *s_out, int64_t lds, int64_t M, int C, int H, void *stream);

/* ---- The optimizer step as two launches over all parameters -----------------------------------------------------------
 * Replaces, per training step (inference/trainer.py:197-204, inference/exponential_moving_average.py:27-32):
 * scaler.unscale_ (non-finite check + g *= 1/scale), clip_grad_norm_ (norms + g *= clip coefficient), the multi-tensor AdamW
 * (torch.optim.AdamW: decoupled weight decay, bias corrections) and the EMA lerp -- with the same arithmetic.
 * chunks: device array of n_chunks records of vsde_optim_chunk_bytes() = 64 bytes:
 *   { float *p, *m, *v, *ema; int32 param, n; int64 goff; int32 group, 0; int64 0 }   (<= vsde_optim_chunk_elems() elements each)
 * grads: device array of the step's gradient base pointers (one per parameter); scale: loss scale (device scalar) or NULL;
 * partials [n_chunks] scratch; tstate [2] = (t_cur, t_next) float step counts, t_next is the persistent one;
 * groups [n_groups][5] doubles = lr, beta1, beta2, eps, weight_decay; max_norm <= 0: no clipping; ema_weight = 1 - decay (< 0: no EMA);
 * out [2] = global gradient norm (unscaled, before clipping), found_inf (0 / 1).  With a loss scale, a non-finite gradient
 * skips the update (parameters, moments and step count unchanged, as GradScaler.step does; the EMA lerp still runs, as the
 * reference's ema.update() does).  Deterministic. */
int vsde_optim_chunk_bytes(void);
int vsde_optim_chunk_elems(void);
int vsde_optim_step(const void *chunks, int n_chunks, const void *grads, const float *scale, float *partials, float *tstate,
                    const double *groups, double max_norm, double ema_weight, float *out, void *stream);

/* ---- Refresh of the cached bf16 GEMM operands after an optimizer step -------------------------------------------------
 * The reference re-casts each nn.Linear weight to bf16 in every forward under autocast (primitives/attn.py:46-54,
 * primitives/mlp.py:41-54); this build keeps the bf16 operands (concatenated / padded / interleaved packs and their
 * transposes) as persistent buffers and re-fills ALL of them with one launch after the optimizer step.
 * tiles: device array of n_tiles records of vsde_pack_tile_bytes() = 64 bytes each:
 *   { const float *src; uint16_t *dst; uint16_t *dst_t; int64_t src_pitch, dst_pitch, pitch_t; int32_t rows, cols; int64_t reserved; }
 * = up to 16 rows x cols of one fp32 parameter row block -> bf16 at dst (row pitch dst_pitch) and, when dst_t != NULL, the
 * same values transposed: dst_t[col * pitch_t + row]. */
int vsde_pack_tile_bytes(void);
int vsde_pack_refresh(const void *tiles, int n_tiles, void *stream);

/* ---- Batched Euler-Maruyama simulator of the MODEL SDE (parameter pre-training stage) --------------------------------
 * Replaces the T-step Python loop of core/euler_maruyama.py:11-45 (called from trainer.py:246-259 with 4096 paths) for
 * SDEs whose drift / diffusion are built in:
 *   VSDE_SDE_OU               f = kappa (mu - x), G = sigma                        examples/ornstein_uhlenbeck.py:18-30
 *   VSDE_SDE_LOTKA_VOLTERRA   analytic 2x2 Cholesky diffusion, three 1e-6 clamps   examples/lotka_volterra.py:18-46
 *   VSDE_SDE_LINEAR_DIAGONAL  f = -a x, G = diag(softplus(b) + 1e-3), theta=(a,b)  (BASELINE.json config 5)
 * x0[B][S], theta[B][P], noise[B][T][S] -> traj[B][T+1][S] with traj[:,0] = x0 and the positive dims (positive_mask: S
 * bytes on the HOST) clamped at 1e-6 after every step.  _bwd: g_traj[B][T+1][S] -> g_x0[B][S], g_theta[B][P] (reverse-mode
 * derivative of exactly that recursion; a clamped entry passes no gradient).  User-defined SDEs keep the torch loop. */
#define VSDE_SDE_OU 1
#define VSDE_SDE_LOTKA_VOLTERRA 2
#define VSDE_SDE_LINEAR_DIAGONAL 3
int vsde_euler_maruyama_fwd(int kind, int B, int T, int S, int P, const float *x0, const float *theta, const float *noise,
                            double time_step, const uint8_t *positive_mask_host, float *traj, void *stream);
int vsde_euler_maruyama_bwd(int kind, int B, int T, int S, int P, const float *theta, const float *noise, const float *traj,
                            const float *g_traj, double time_step, const uint8_t *positive_mask_host, float *g_x0,
                            float *g_theta, void *stream);

/* Forecast of a built-in SDE: the recursion of vsde_euler_maruyama_fwd (same step, same 1e-6 clamp of the positive dims, NaN
 * passed through) run for T steps from x_start[B][S] with theta[B][P], keeping only the states after the K grid steps
 * out_steps[K] (device int32, non-decreasing, values in 1..T, duplicates allowed) in out[B][K][S]; an entry above T reads NaN.
 * The Gaussian increments are made in the kernel, so neither the noise nor the trajectory exists in memory (O(B K S)).
 * Noise stream: the normal of path b, step t, dim i is number t % 4 of philox4x32_10(counter {t / 4, i, b, 0},
 * key {key[0], key[1]}) (Random123), Box-Muller on the word pairs (w0, w1) -> (z0, z1) and (w2, w3) -> (z2, z3):
 *   u = ((w >> 8) + 0.5) 2^-24 in fp32 (round to nearest even: u in (0, 1]),  r = sqrt(-2 ln u_a),
 *   z_a = r cos(2 pi u_b),  z_b = r sin(2 pi u_b).
 * The tails are cut at |z| <= sqrt(50 ln 2) ~ 5.89 sigma.  key: 2 words in DEVICE memory, read by the kernel, so a launch captured
 * in a HIP graph takes a fresh key per replay.  Kinds 1, 2: a thread per path; kind 3 (S <= 32): a thread per (path, dim).
 * Forward only (no gradient). */
int vsde_forecast(int kind, int B, int T, int S, int P, int K, const float *x_start, const float *theta, const int *out_steps,
                  const uint32_t *key, double time_step, const uint8_t *positive_mask_host, float *out, void *stream);

/* The [B]-sized tail of the ELBO (inference/evidence_lower_bound.py:52-83): Gaussian observation log-density of the states at
 * the K observed grid points x_obs[B][K][S] (core/observations.py:57-74; obs_matrix [O][S] or NULL = identity), iid prior
 * (prior_type 0 Normal, 1 LogNormal; core/priors.py:46-60), mean-field posterior log q(theta)
 * (models/sde_parameter_posterior.py:44-66; theta_positive_mask_host: P bytes), combined with the three path terms into
 *   out6 = [mean_b(obs + sde - gen + jac + prior - post), mean obs, mean sde, mean gen, mean prior, mean post].
 * _bwd: upstream gradient of out6 -> gradients of x_obs, theta, the posterior's mean / log_std [P] and the three path terms
 * [B].  One single-workgroup kernel each; dims S, O, P <= 16. */
int vsde_elbo_tail_fwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values, const float *obs_matrix,
                       double variance, const float *theta, int prior_type, double prior_mean, double prior_std,
                       const float *post_mean, const float *post_log_std, const uint8_t *theta_positive_mask_host,
                       const float *sde_lp, const float *gen_lp, const float *log_jac, float *out6, void *stream);
int vsde_elbo_tail_bwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values, const float *obs_matrix,
                       double variance, const float *theta, int prior_type, double prior_mean, double prior_std,
                       const float *post_mean, const float *post_log_std, const uint8_t *theta_positive_mask_host,
                       const float *g_out6, float *g_x_obs, float *g_theta, float *g_post_mean, float *g_post_log_std,
                       float *g_sde, float *g_gen, float *g_jac, void *stream);

/* Count observation terms (core/observations.py: PoissonObservationLikelihood, NegativeBinomialObservationLikelihood).  The
 * vsde_*count_* entry points mirror the entry point named after them with (lik_kind, scale, dispersion, row_const) in place of
 * variance: lambda_o = max(scale (H x)_o, 1e-6) (torch.clamp: NaN propagates, no gradient where scale (H x)_o < 1e-6) and, per
 * observed count y = obs_values[k][o],
 *   VSDE_LIK_POISSON            log p = y log lambda - lambda - lgamma(y + 1)
 *   VSDE_LIK_NEGATIVE_BINOMIAL  log p = lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log(r / (r + lambda)) + y log(lambda / (r + lambda))
 * with r = dispersion > 0 (mean lambda, variance lambda + lambda^2 / r; ignored for Poisson).  The kernels evaluate the deviance
 * form  y log(lambda / y) - (lambda - y)  resp.  y log(lambda / y) - (r + y) log((r + lambda) / (r + y))  (the y log term absent
 * at y = 0) and add row_const[k] (DEVICE memory, K floats), the sum over o of the terms of y alone, which the caller computes:
 *   Poisson  y log y - y - lgamma(y + 1);   NB  lgamma(y + r) - lgamma(r) - lgamma(y + 1) + r log r + y log y - (r + y) log(r + y).
 * The same argument checks as the mirrored entry point, before any HIP call; in addition VSDE_E_BADARG for an unknown lik_kind,
 * scale <= 0, dispersion <= 0 for the negative binomial, or row_const NULL while K > 0.  The counts are not checked (a negative
 * or fractional y gives the formula's value). */
#define VSDE_LIK_POISSON 1
#define VSDE_LIK_NEGATIVE_BINOMIAL 2
int vsde_count_elbo_tail_fwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values, const float *obs_matrix,
                             int lik_kind, double scale, double dispersion, const float *row_const, const float *theta,
                             int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std,
                             const uint8_t *theta_positive_mask_host, const float *sde_lp, const float *gen_lp, const float *log_jac,
                             float *out6, void *stream);
int vsde_count_elbo_tail_bwd(int B, int K, int S, int O, int P, const float *x_obs, const float *obs_values, const float *obs_matrix,
                             int lik_kind, double scale, double dispersion, const float *row_const, const float *theta,
                             int prior_type, double prior_mean, double prior_std, const float *post_mean, const float *post_log_std,
                             const uint8_t *theta_positive_mask_host, const float *g_out6, float *g_x_obs, float *g_theta,
                             float *g_post_mean, float *g_post_log_std, float *g_sde, float *g_gen, float *g_jac, void *stream);

/* Importance log-weights of posterior draws (VariationalPosterior.log_evidence): per sample b the ELBO integrand
 *   log_w[b] = obs + sum_t (sde_t - gen_t + jac_t) + prior - post
 * of vsde_elbo_path_terms + vsde_elbo_tail_fwd before their batch means, in one pass.  z[B][T+1][S] latent paths (softplus on
 * the positive state dims: state_positive_mask_host, S bytes), means[B][T][S], chol[B][T][S][S] of the generating head,
 * theta[B][P]; the observation states are read from z at the grid rows obs_rows[K] (device int32).  kind 1..3: drift /
 * diffusion of the built-in SDE (VSDE_SDE_*) evaluated in registers (drift / diffusion may be NULL); kind 0: the caller's
 * drift[B][T][S], diffusion[B][T][S][S].  Other arguments as vsde_elbo_tail_fwd.  S, O, P <= 16 (S beyond: VSDE_E_STATE). */
int vsde_log_weights(int kind, int B, int T, int S, int K, int O, int P, const float *z, const float *means, const float *chol,
                     const float *drift, const float *diffusion, const float *theta, const int *obs_rows, const float *obs_values,
                     const float *obs_matrix, double variance, int prior_type, double prior_mean, double prior_std,
                     const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host,
                     const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream);
/* vsde_log_weights with a count observation term (see vsde_count_elbo_tail_fwd). */
int vsde_count_log_weights(int kind, int B, int T, int S, int K, int O, int P, const float *z, const float *means, const float *chol,
                           const float *drift, const float *diffusion, const float *theta, const int *obs_rows,
                           const float *obs_values, const float *obs_matrix, int lik_kind, double scale, double dispersion,
                           const float *row_const, int prior_type, double prior_mean, double prior_std, const float *post_mean,
                           const float *post_log_std, const uint8_t *state_positive_mask_host,
                           const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream);
/* Merge the first n entries of log_w into the running fp64 state (device memory, 6 doubles; start from
 * [-inf, 0, 0, 0, 0, 0]):  [M, sum exp(lw - M), sum exp(2 (lw - M)), sum lw, n, n_nonfinite], M the running max.  One
 * single-workgroup launch per chunk, no host synchronisation, bitwise deterministic.  NaN / +inf entries count in n_nonfinite
 * and n only; -inf entries are zero weights. */
int vsde_log_weight_accumulate(int n, const float *log_w, double *state6, void *stream);

/* Drift and diffusion factor of a built-in SDE on every grid point of a batch of paths -- what the ELBO evaluates through the
 * user's Python callables on the flattened [(B T), S] states (inference/evidence_lower_bound.py:37-40) -- and the
 * vector-Jacobian product its backward needs.  x[B][T+1][S] (rows 0..T-1 are read), theta[B][P] -> drift[B][T][S],
 * diffusion[B][T][S][S].  _bwd: g_drift, g_diffusion -> g_x[B][T+1][S] (row T zero), g_theta[B][P] (sum over t in a fixed
 * order).  torch.clamp(min=1e-6) semantics: the gradient passes where the clamped quantity is >= the bound. */
int vsde_sde_coefficients_fwd(int kind, int B, int T, int S, int P, const float *x, const float *theta, float *drift,
                              float *diffusion, void *stream);
int vsde_sde_coefficients_bwd(int kind, int B, int T, int S, int P, const float *x, const float *theta, const float *g_drift,
                              const float *g_diffusion, float *g_x, float *g_theta, void *stream);

/* Mass-action chemical reaction networks in their diffusion (chemical Langevin) approximation (ReactionNetworkSDE): S species,
 * R reactions, one rate constant per reaction (theta[B][R], so P = R).  With r_ji = order[j][i] and nu_ji = change[j][i]:
 *   propensity  h_j = theta_j prod_i x_i^r_ji   (no combinatorial factor: such constants belong in theta_j)
 *   drift       f = sum_j h_j nu_j,   covariance  Sigma = sum_j h_j nu_j nu_j^T,
 *   diffusion   the floored Cholesky factor of Sigma, column by column:
 *               L_jj = sqrt(max(Sigma_jj - sum_{k<j} L_jk^2, 1e-6)),  L_ij = (Sigma_ij - sum_{k<j} L_ik L_jk) / max(L_jj, 1e-6)
 * with torch.clamp semantics (NaN propagates; the gradient passes where the clamped quantity is >= 1e-6).  At S = 2 these are
 * the three clamps of VSDE_SDE_LOTKA_VOLTERRA.  The descriptor is HOST memory, copied into the kernel arguments at launch: no
 * device allocation, so every vsde_crn_* call can be captured in a HIP graph.  Entries of rows >= R and columns >= S are
 * ignored.  Each vsde_crn_* entry point takes the arguments of the entry point it mirrors with `kind` replaced by the
 * descriptor, and returns VSDE_E_BADARG before any HIP call when the descriptor is bad (S outside 1..8, R outside 1..16, an
 * order outside 0..3) or disagrees with S / P. */
#define VSDE_SDE_REACTION_NETWORK 4
#define VSDE_CRN_MAX_SPECIES 8
#define VSDE_CRN_MAX_REACTIONS 16
#define VSDE_CRN_MAX_ORDER 3
typedef struct vsde_crn_network {
    int32_t S;                                                     /* species = state_dim                      */
    int32_t R;                                                     /* reactions = sde_param_dim                */
    int8_t order[VSDE_CRN_MAX_REACTIONS][VSDE_CRN_MAX_SPECIES];   /* reactant order r_ji of species i, 0..3   */
    int8_t change[VSDE_CRN_MAX_REACTIONS][VSDE_CRN_MAX_SPECIES];  /* net change nu_ji = products - reactants   */
} vsde_crn_network;
int vsde_crn_sde_coefficients_fwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *x, const float *theta,
                                  float *drift, float *diffusion, void *stream);
int vsde_crn_sde_coefficients_bwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *x, const float *theta,
                                  const float *g_drift, const float *g_diffusion, float *g_x, float *g_theta, void *stream);
int vsde_crn_euler_maruyama_fwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *x0, const float *theta,
                                const float *noise, double time_step, const uint8_t *positive_mask_host, float *traj, void *stream);
int vsde_crn_euler_maruyama_bwd(const vsde_crn_network *net, int B, int T, int S, int P, const float *theta, const float *noise,
                                const float *traj, const float *g_traj, double time_step, const uint8_t *positive_mask_host,
                                float *g_x0, float *g_theta, void *stream);
/* The noise stream of vsde_forecast (the same normals for the same key, path, step and dim). */
int vsde_crn_forecast(const vsde_crn_network *net, int B, int T, int S, int P, int K, const float *x_start, const float *theta,
                      const int *out_steps, const uint32_t *key, double time_step, const uint8_t *positive_mask_host, float *out,
                      void *stream);
/* vsde_log_weights with the network's drift / diffusion evaluated in registers (no drift / diffusion tensors). */
int vsde_crn_log_weights(const vsde_crn_network *net, int B, int T, int S, int K, int O, int P, const float *z, const float *means,
                         const float *chol, const float *theta, const int *obs_rows, const float *obs_values,
                         const float *obs_matrix, double variance, int prior_type, double prior_mean, double prior_std,
                         const float *post_mean, const float *post_log_std, const uint8_t *state_positive_mask_host,
                         const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream);
/* vsde_crn_log_weights with a count observation term (see vsde_count_elbo_tail_fwd). */
int vsde_crn_count_log_weights(const vsde_crn_network *net, int B, int T, int S, int K, int O, int P, const float *z,
                               const float *means, const float *chol, const float *theta, const int *obs_rows,
                               const float *obs_values, const float *obs_matrix, int lik_kind, double scale, double dispersion,
                               const float *row_const, int prior_type, double prior_mean, double prior_std, const float *post_mean,
                               const float *post_log_std, const uint8_t *state_positive_mask_host,
                               const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream);

/* Rate laws of a reaction network (ReactionNetworkSDE(rate_laws=..., rate_constants=...)).  Reaction j follows law[j]:
 *   VSDE_CRN_LAW_MASS_ACTION      h_j = k_j prod_i x_i^r_ji                     (modifier / hill_n ignored)
 *   VSDE_CRN_LAW_HILL_ACTIVATION  h_j = k_j u^n / (K_j^n + u^n)
 *   VSDE_CRN_LAW_HILL_REPRESSION  h_j = k_j K_j^n / (K_j^n + u^n)
 * with u = max(x_s, 0) of the modifier species s = modifier[j] (torch.clamp semantics: NaN propagates, the gradient reaches x_s
 * where x_s >= 0) and n = hill_n[j] in 1..4; powers by repeated multiplication.  The reactant row of a rate-law reaction sets
 * its net change only.  Drift, covariance and diffusion are built from the h_j as for vsde_crn_network.  The vsde_crn_kinetic_*
 * entry points take, in place of theta, the effective constants rates[B][2R] = (k_0 .. k_{R-1}, K_0 .. K_{R-1}) (so P = 2R;
 * K_j is ignored for mass-action reactions), and the network and rate-law descriptors (HOST memory, copied into the kernel
 * arguments: capturable).  They return VSDE_E_BADARG before any HIP call for a bad network descriptor, a law code outside
 * 0..2, a modifier outside 0..S-1 or a Hill coefficient outside 1..4 on a rate-law reaction, or P != 2R.  Entries of rows
 * >= R are ignored. */
#define VSDE_CRN_LAW_MASS_ACTION 0
#define VSDE_CRN_LAW_HILL_ACTIVATION 1
#define VSDE_CRN_LAW_HILL_REPRESSION 2
#define VSDE_CRN_MAX_HILL 4
typedef struct vsde_crn_kinetics {
    int8_t law[VSDE_CRN_MAX_REACTIONS];       /* VSDE_CRN_LAW_*                        */
    int8_t modifier[VSDE_CRN_MAX_REACTIONS];  /* modifier species s_j of a rate law     */
    int8_t hill_n[VSDE_CRN_MAX_REACTIONS];    /* Hill coefficient n_j of a rate law     */
} vsde_crn_kinetics;
int vsde_crn_kinetic_sde_coefficients_fwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int P,
                                          const float *x, const float *rates, float *drift, float *diffusion, void *stream);
int vsde_crn_kinetic_sde_coefficients_bwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int P,
                                          const float *x, const float *rates, const float *g_drift, const float *g_diffusion,
                                          float *g_x, float *g_rates, void *stream);
int vsde_crn_kinetic_euler_maruyama_fwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int P,
                                        const float *x0, const float *rates, const float *noise, double time_step,
                                        const uint8_t *positive_mask_host, float *traj, void *stream);
int vsde_crn_kinetic_euler_maruyama_bwd(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int P,
                                        const float *rates, const float *noise, const float *traj, const float *g_traj,
                                        double time_step, const uint8_t *positive_mask_host, float *g_x0, float *g_rates,
                                        void *stream);
int vsde_crn_kinetic_forecast(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int P, int K,
                              const float *x_start, const float *rates, const int *out_steps, const uint32_t *key,
                              double time_step, const uint8_t *positive_mask_host, float *out, void *stream);
/* P here is the width of theta [B][P] (the prior / posterior terms); R_eff = 2R is the width of rates [B][2R] (the drift and
 * diffusion). */
int vsde_crn_kinetic_log_weights(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int K, int O,
                                 int P, int R_eff, const float *z, const float *means, const float *chol, const float *theta,
                                 const float *rates, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                 double variance, int prior_type, double prior_mean, double prior_std, const float *post_mean,
                                 const float *post_log_std, const uint8_t *state_positive_mask_host,
                                 const uint8_t *theta_positive_mask_host, double time_step, float *log_w, void *stream);
/* vsde_crn_kinetic_log_weights with a count observation term (see vsde_count_elbo_tail_fwd). */
int vsde_crn_kinetic_count_log_weights(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int T, int S, int K, int O,
                                       int P, int R_eff, const float *z, const float *means, const float *chol, const float *theta,
                                       const float *rates, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                       int lik_kind, double scale, double dispersion, const float *row_const, int prior_type,
                                       double prior_mean, double prior_std, const float *post_mean, const float *post_log_std,
                                       const uint8_t *state_positive_mask_host, const uint8_t *theta_positive_mask_host,
                                       double time_step, float *log_w, void *stream);

/* Bootstrap particle filter: log p^(y | theta_m) of the Euler-Maruyama-discretised built-in SDE with the Gaussian observation
 * term of vsde_elbo_tail_fwd, for M parameter vectors at once (viforsdes_amd/inference/particle_filter.py is the specification).
 * One workgroup per theta, one thread per particle: N particles, a multiple of 64 up to 1024 (reaction networks of 5..8 species:
 * up to 512); S <= 16 (kinds 1, 2 and networks: their own S), O <= 16, M N < 2^32.  x0[M][S] start states (every particle of filter
 * m starts there), theta[M][P], obs_rows[K] (device int32, non-decreasing grid rows; the run has obs_rows[K-1] steps, several
 * observations may share a row), obs_values[K][O], obs_matrix[O][S] or NULL (identity, O == S), key: 2 words in DEVICE memory.
 *   Between observations: the step and 1e-6 clamp of vsde_euler_maruyama_fwd.  Noise: the stream of vsde_forecast; the normal of
 * filter m, particle slot j, GLOBAL grid step t, dim i is that of path b = m N + j (counter word 3 = 0): a slot keeps its stream
 * across resampling.
 *   At observation k: lw_j = sum_o -(y_ko - (H x_j)_o)^2 / (2 variance) - log(2 pi variance) / 2, NaN counts as -inf;
 * increments[m][k] = max lw + log sum_j exp(lw_j - max) - log N; ess[m][k] = (sum w)^2 / sum w^2 with w_j = exp(lw_j - max);
 * filtered_mean / filtered_std [m][k][S]: weighted mean and standard deviation of the particles BEFORE resampling;
 * particles [m][k][N][S] (those states) and ancestors [m][k][N] are optional (NULL = not written).  Then systematic resampling, at
 * every observation: inclusive cumulative sums C_j of w in particle order (made non-decreasing by a running maximum: a tree of fp32
 * sums is not), u = ((w0 >> 8) + 0.5) 2^-24 in (0, 1] with w0 the first word of philox4x32_10(counter {k, 0, m, 1}, key),
 * tau_j = (j + u) / N C_{N-1}, ancestor_j = min(#{i : C_i <= tau_j}, N - 1); particle j continues from the state of ancestor_j.
 * If no weight is positive: increment -inf, ess 0, mean / std NaN, ancestors the identity, the particles stay as they are.
 * log_likelihood[m] = sum_k increments[m][k].  VSDE_E_BADARG before any HIP call for N not a multiple of 64 or above the limit, S
 * or O above 16, K < 1, O != S without obs_matrix, or a bad network / rate-law descriptor.  The vsde_crn_* forms take the
 * descriptors as the other vsde_crn_* entry points do (rates[M][2R] in place of theta for the rate-law form).  Forward only. */
int vsde_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta, const int *obs_rows,
                         const float *obs_values, const float *obs_matrix, double variance, const uint32_t *key, double time_step,
                         const uint8_t *positive_mask_host, float *log_likelihood, float *increments, float *ess,
                         float *filtered_mean, float *filtered_std, float *particles, int *ancestors, void *stream);
int vsde_crn_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                             const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                             double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                             float *log_likelihood, float *increments, float *ess, float *filtered_mean, float *filtered_std,
                             float *particles, int *ancestors, void *stream);
int vsde_crn_kinetic_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P, int K,
                                     int O, const float *x0, const float *rates, const int *obs_rows, const float *obs_values,
                                     const float *obs_matrix, double variance, const uint32_t *key, double time_step,
                                     const uint8_t *positive_mask_host, float *log_likelihood, float *increments, float *ess,
                                     float *filtered_mean, float *filtered_std, float *particles, int *ancestors, void *stream);

/* The bootstrap filter with a count observation term (see vsde_count_elbo_tail_fwd): vsde_particle_filter where only the log-weight
 * at an observation differs, lw_j = row_const[k] + sum_o deviance term of (y_ko, lambda_o(x_j)), NaN as -inf; propagation, noise
 * stream, increments, moments and resampling are the same code.  Particle limits: as vsde_particle_filter. */
int vsde_count_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                               const int *obs_rows, const float *obs_values, const float *obs_matrix, int lik_kind, double scale,
                               double dispersion, const float *row_const, const uint32_t *key, double time_step,
                               const uint8_t *positive_mask_host, float *log_likelihood, float *increments, float *ess,
                               float *filtered_mean, float *filtered_std, float *particles, int *ancestors, void *stream);
int vsde_crn_count_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                   const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                   int lik_kind, double scale, double dispersion, const float *row_const, const uint32_t *key,
                                   double time_step, const uint8_t *positive_mask_host, float *log_likelihood, float *increments,
                                   float *ess, float *filtered_mean, float *filtered_std, float *particles, int *ancestors,
                                   void *stream);
int vsde_crn_kinetic_count_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                           int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                           const float *obs_values, const float *obs_matrix, int lik_kind, double scale,
                                           double dispersion, const float *row_const, const uint32_t *key, double time_step,
                                           const uint8_t *positive_mask_host, float *log_likelihood, float *increments, float *ess,
                                           float *filtered_mean, float *filtered_std, float *particles, int *ancestors,
                                           void *stream);

/* Guided particle filter (proposal = "bridge": the modified diffusion bridge, viforsdes_amd/inference/particle_filter.py is the
 * specification): vsde_particle_filter with every Euler step drawn from a Gaussian pulled towards the next observation and the
 * ratio model / proposal carried in the log-weight, so log p^ stays unbiased.  Same arguments, same checks, same noise stream and
 * the same rules from the log-weight on; in addition S <= 4 and O <= 4 (VSDE_E_BADARG otherwise).  Step t -> t + 1 of a particle
 * at x, with k the first observation whose row exceeds t, n = obs_rows[k] - t, f / G the drift / diffusion factor at x:
 * A = sqrt(time_step) H G, psi = n A A^T + variance I = R R^T, W = R^-1 A, r = R^-1 (y_k - H (x + n time_step f)), m = W^T r,
 * C = I - W^T W = M M^T (lower factor, every pivot floored at 1e-6 before its square root), eps = m + M z with z the stream's
 * normals of the step, x' = x + f time_step + sqrt(time_step) G eps, then the 1e-6 clamp; lr += -|eps|^2 / 2 + |z|^2 / 2 +
 * sum_j log M_jj.  At observation k: lw_j = lr_j + the Gaussian term of vsde_particle_filter, then lr = 0.
 * log_weights [m][k][N] (those lw) is optional like particles (NULL = not written). */
int vsde_guided_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                                const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                const uint32_t *key, double time_step, const uint8_t *positive_mask_host, float *log_likelihood,
                                float *increments, float *ess, float *filtered_mean, float *filtered_std, float *particles,
                                int *ancestors, float *log_weights, void *stream);
int vsde_crn_guided_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                    const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                    double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                    float *log_likelihood, float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                    float *particles, int *ancestors, float *log_weights, void *stream);
int vsde_crn_kinetic_guided_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                            int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                            const float *obs_values, const float *obs_matrix, double variance, const uint32_t *key,
                                            double time_step, const uint8_t *positive_mask_host, float *log_likelihood,
                                            float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                            float *particles, int *ancestors, float *log_weights, void *stream);

/* Replay of a filter's genealogy: D smoothed paths x_{0:T} | y, theta_m per filter from what vsde_particle_filter /
 * vsde_count_particle_filter stored (viforsdes_amd/inference/particle_smoother.py is the specification).  particles[M][K][N][S] and
 * ancestors[M][K][N] are that call's outputs, and kind / descriptors, M, N, S, P, K, O, x0, theta (rates), obs_rows, key, time_step
 * and positive_mask_host must be that call's too; last_slot[M][D] (device int32) is the slot of each draw at the LAST observation
 * (the caller draws it from the final weights), -1 for a filter without a smoothing sample; T = obs_rows[K-1], the steps of a path.
 *   One launch, one thread per (k, m, d): lineage[m][d][K-1] = last_slot[m][d], lineage[m][d][k-1] = ancestors[m][k-1][lineage[m][d][k]]
 * (written when lineage is not NULL), and segment k, the grid steps obs_rows[k-1] .. obs_rows[k] - 1 (from 0 for k = 0), is run
 * again from particles[m][k-1][lineage[m][d][k-1]] (x0[m] for k = 0) with the normals of path b = m N + lineage[m][d][k], the step
 * and 1e-6 clamp of vsde_particle_filter: the state after step t goes to paths[m][d][t+1][S], paths[m][d][0] = x0[m].  The replay of
 * a bootstrap filter does not depend on the observation term, so the count filters share these entry points.  A draw with
 * last_slot < 0: lineage -1, paths NaN.  A segment whose rows decrease or pass T is not written.
 *   VSDE_E_BADARG before any HIP call: the checks of vsde_particle_filter on N, S, O, K; D < 1, T < 0, M D K >= 2^31, a NULL
 * argument other than lineage.  No particle limit below 1024 applies: a replay thread is not tied to a particle. */
int vsde_filter_replay(int kind, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0, const float *theta,
                       const int *obs_rows, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                       const float *particles, const int *ancestors, const int *last_slot, float *paths, int *lineage, void *stream);
int vsde_crn_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0,
                           const float *theta, const int *obs_rows, const uint32_t *key, double time_step,
                           const uint8_t *positive_mask_host, const float *particles, const int *ancestors, const int *last_slot,
                           float *paths, int *lineage, void *stream);
int vsde_crn_kinetic_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P, int K, int O,
                                   int D, int T, const float *x0, const float *rates, const int *obs_rows, const uint32_t *key,
                                   double time_step, const uint8_t *positive_mask_host, const float *particles, const int *ancestors,
                                   const int *last_slot, float *paths, int *lineage, void *stream);

/* vsde_filter_replay for what vsde_guided_particle_filter stored: segment k repeats the bridge steps towards obs_values[k] (n =
 * obs_rows[k] - t steps ahead), so obs_values[K][O], obs_matrix[O][S] or NULL and variance must be that call's as well.  S <= 4 and
 * O <= 4 (VSDE_E_BADARG otherwise, before any HIP call). */
int vsde_guided_filter_replay(int kind, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0, const float *theta,
                              const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                              const uint32_t *key, double time_step, const uint8_t *positive_mask_host, const float *particles,
                              const int *ancestors, const int *last_slot, float *paths, int *lineage, void *stream);
int vsde_crn_guided_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0,
                                  const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                  double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                  const float *particles, const int *ancestors, const int *last_slot, float *paths, int *lineage,
                                  void *stream);
int vsde_crn_kinetic_guided_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P, int K,
                                          int O, int D, int T, const float *x0, const float *rates, const int *obs_rows,
                                          const float *obs_values, const float *obs_matrix, double variance, const uint32_t *key,
                                          double time_step, const uint8_t *positive_mask_host, const float *particles,
                                          const int *ancestors, const int *last_slot, float *paths, int *lineage, void *stream);

/* Metropolis step of particle marginal Metropolis-Hastings (viforsdes_amd/inference/particle_mcmc.py is the specification): C
 * independent chains over u [P] (theta with a log taken on the positive dims), a thread per chain, R filter estimates per chain.
 * One launch CLOSES iteration `iteration - 1` and OPENS iteration `iteration`; the caller runs the particle filter on
 * theta_prop[C*R][P] with filter_key between two launches and hands its log_likelihood [C][R] to the next one as loglik_prop.
 *   Close (skipped when loglik_prop is NULL), it = iteration - 1: ll' = log mean_r exp(loglik_prop[c][r]) (NaN if any is NaN, -inf
 * if all are -inf); target' = prop_log_prior[c] + ll'; log_u = log(((w0 >> 8) + 0.5) 2^-24) with w0 the first word of
 * philox4x32_10({it, 0, c, 4}, key); accepted iff target' is not NaN and (it == 0 or (target' != -inf and log_u < target' -
 * cur_log_target[c])).  On acceptance cur_u[c] = prop_u[c], cur_log_target[c] = target', cur_loglik[c] = ll', n_accept[c] += 1.
 * Then, where not NULL, sample_row[c][P] = theta of cur_u[c] (exp on the positive dims), loglik_row[c], target_row[c] = the
 * carried values.
 *   Open: for iteration > 0, u'_i = cur_u[c][i] + step_size sum_{j <= i} scale_tril[i][j] z_j with z_j the Box-Muller normal j & 3
 * of philox4x32_10({iteration, j >> 2, c, 3}, key) (the rule of vsde_forecast: word pairs (w0, w1), (w2, w3)), written to
 * prop_u[c]; iteration 0 proposes prop_u[c] as the caller gave it.  theta' = u' with exp on the positive dims, R copies of it to
 * theta_prop[c R + r]; prop_log_prior[c] = the prior's log density of theta' (prior_type 0: Normal, 1: LogNormal, iid over P, as
 * vsde_elbo_tail_fwd) + sum over the positive dims of u'_i; filter_key = the first two words of philox4x32_10({iteration, 0, 0,
 * 5}, key).  Counter words 3, 4, 5 in the fourth slot: 0, 1, 2 are the path normals, the resampling uniforms and the smoother.
 *   scale_tril [P][P] is read on the HOST (it travels in the kernel's argument block) and so is theta_positive_mask_host; every
 * other pointer is device memory.  VSDE_E_BADARG before any HIP call: C, R < 1, iteration < 0, P outside 1..16, C R P >= 2^31, a
 * NULL pointer other than loglik_prop / sample_row / loglik_row / target_row, loglik_prop given at iteration 0, step_size or
 * prior_std not positive, prior_type not 0 / 1, scale_tril not finite, not lower triangular or with a diagonal entry <= 0. */
int vsde_pmmh_step(int C, int P, int R, int iteration, const float *scale_tril, double step_size, int prior_type, double prior_mean,
                   double prior_std, const uint8_t *theta_positive_mask_host, const uint32_t *key, const float *loglik_prop,
                   float *cur_u, float *cur_log_target, float *cur_loglik, float *prop_u, float *prop_log_prior, float *theta_prop,
                   uint32_t *filter_key, float *sample_row, float *loglik_row, float *target_row, int *n_accept, void *stream);

/* vsde_pmmh_step for chains that carry a latent path with their state (PMMH as a sampler of p(theta, x_{0:T} | y)): the same launch,
 * every output of vsde_pmmh_step bit for bit, and for a chain ACCEPTED in the close half the record of the proposal's path, drawn
 * from what the filter launch of iteration it = iteration - 1 stored: particles[C R][K][N][S] (states before resampling) and
 * ancestors[C R][K][N] (filter m = c R + r, N particles, K observations).
 *   Filter: w_r = exp(loglik_prop[c][r] - max_r), C_r its inclusive sums in r order, v0 and v1 the uniforms ((w >> 8) + 0.5) 2^-24
 * of the first and second word of philox4x32_10({it, 0, c, 6}, key), r* = min(#{r : C_r <= v0 C_{R-1}}, R - 1), m* = c R + r*.
 * Slot: J = min(floor(v1 N), N - 1) (the fp32 product), lineage[K-1] = ancestors[m*][K-1][J] (a uniformly chosen offspring slot of
 * the filter's own last resampling has an ancestor drawn from the final weights), lineage[k-1] = ancestors[m*][k-1][lineage[k]],
 * every entry clamped into [0, N - 1].  Record: cur_anchor[c][k][S] = particles[m*][k][lineage[k]], cur_noise_path[c][k] = m* N +
 * lineage[k], cur_path_iteration[c] = it.  Where every estimate is -inf (iteration 0 accepts such a proposal) the record is dead:
 * noise paths 0xFFFFFFFF, anchors NaN.  A rejected chain keeps its record.  Then, where not NULL, anchor_row[C][K][S],
 * noise_row[C][K] and iteration_row[C] receive the carried record of every chain.  Counter word 6 in the fourth slot is new.
 *   VSDE_E_BADARG before any HIP call: those of vsde_pmmh_step; N, K or S < 1, C R N >= 2^32, a NULL pointer among particles,
 * ancestors, cur_anchor, cur_noise_path, cur_path_iteration. */
int vsde_pmmh_step_paths(int C, int P, int R, int iteration, const float *scale_tril, double step_size, int prior_type,
                         double prior_mean, double prior_std, const uint8_t *theta_positive_mask_host, const uint32_t *key,
                         const float *loglik_prop, float *cur_u, float *cur_log_target, float *cur_loglik, float *prop_u,
                         float *prop_log_prior, float *theta_prop, uint32_t *filter_key, float *sample_row, float *loglik_row,
                         float *target_row, int *n_accept, int N, int K, int S, const float *particles, const int *ancestors,
                         float *cur_anchor, uint32_t *cur_noise_path, int *cur_path_iteration, float *anchor_row, uint32_t *noise_row,
                         int *iteration_row, void *stream);

/* Replay of B path records of vsde_pmmh_step_paths: paths[B][T+1][S] on the grid, T = obs_rows[K-1].  Record b brings x0[b][S],
 * theta[b][P] (rates), anchors[b][K][S], noise_path[b][K] and its own filter key keys[b][2]; kind / descriptors, S, P, K, O,
 * obs_rows, time_step and positive_mask_host are those of the filter launches the records were drawn from.  One launch, a thread
 * per (k, b): segment k, the grid steps obs_rows[k-1] .. obs_rows[k] - 1 (from 0 for k = 0), starts at anchors[b][k-1] (x0[b] for
 * k = 0) and takes the normals of path noise_path[b][k] under keys[b], with the step and 1e-6 clamp of vsde_particle_filter: the
 * state after step t goes to paths[b][t+1], paths[b][0] = x0[b].  A record with noise_path[b][K-1] = 0xFFFFFFFF is dead: paths NaN.
 * A segment whose rows decrease or pass T is not written.
 *   VSDE_E_BADARG before any HIP call: B, K < 1, S or O outside 1..16, T < 0, B K >= 2^31, time_step <= 0, a NULL argument. */
int vsde_anchored_replay(int kind, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta, const int *obs_rows,
                         const float *anchors, const uint32_t *noise_path, const uint32_t *keys, double time_step,
                         const uint8_t *positive_mask_host, float *paths, void *stream);
int vsde_crn_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta,
                             const int *obs_rows, const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                             double time_step, const uint8_t *positive_mask_host, float *paths, void *stream);
int vsde_crn_kinetic_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K, int O, int T,
                                     const float *x0, const float *rates, const int *obs_rows, const float *anchors,
                                     const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                     const uint8_t *positive_mask_host, float *paths, void *stream);

/* vsde_anchored_replay for records drawn from vsde_guided_particle_filter launches: segment k repeats the bridge steps towards
 * obs_values[k], so obs_values[K][O], obs_matrix[O][S] or NULL and variance must be those launches' as well.  S <= 4 and O <= 4
 * (VSDE_E_BADARG otherwise, before any HIP call). */
int vsde_guided_anchored_replay(int kind, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta,
                                const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                const float *anchors, const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                const uint8_t *positive_mask_host, float *paths, void *stream);
int vsde_crn_guided_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int O, int T, const float *x0,
                                    const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                    double variance, const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                    double time_step, const uint8_t *positive_mask_host, float *paths, void *stream);
int vsde_crn_kinetic_guided_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K, int O,
                                            int T, const float *x0, const float *rates, const int *obs_rows, const float *obs_values,
                                            const float *obs_matrix, double variance, const float *anchors,
                                            const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                            const uint8_t *positive_mask_host, float *paths, void *stream);

/* Residual-bridge proposal (proposal = "residual_bridge": Whitaker, Golightly, Boys and Sherlock 2017;
 * viforsdes_amd/inference/particle_filter.py is the specification): the nine guided entry points above with ONE quantity of the
 * step replaced.  A particle carries a deterministic companion path eta: at the start of a segment (obs_rows[k-1], or 0, when
 * there are steps towards observation k) eta = x, and a first pass runs the noise-free Euler scheme eta <- clamp(eta + time_step
 * f(eta)) over the segment's obs_rows[k] - t0 steps; its end is eta_end.  In the step t -> t + 1 the residual of the guided step
 * becomes y_k - H (eta_end + (x - eta) + n time_step (f(x) - f(eta))); A, psi, W, m, C, M, eps, x', the clamp and lr are those of
 * vsde_guided_particle_filter with the same normals; then eta <- clamp(eta + time_step f(eta)).  Same arguments, same checks before
 * any HIP call, same outputs and the same S <= 4, O <= 4; the particle limit is pf_max_n's residual rule (today the guided one:
 * 512 at S = 4).  The replays restart every segment from its stored start state, so they form the same eta and repeat the filter's
 * states bit for bit. */
int vsde_residual_particle_filter(int kind, int M, int N, int S, int P, int K, int O, const float *x0, const float *theta,
                                  const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                  const uint32_t *key, double time_step, const uint8_t *positive_mask_host, float *log_likelihood,
                                  float *increments, float *ess, float *filtered_mean, float *filtered_std, float *particles,
                                  int *ancestors, float *log_weights, void *stream);
int vsde_crn_residual_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const float *x0,
                                      const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                      double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                      float *log_likelihood, float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                      float *particles, int *ancestors, float *log_weights, void *stream);
int vsde_crn_kinetic_residual_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                              int K, int O, const float *x0, const float *rates, const int *obs_rows,
                                              const float *obs_values, const float *obs_matrix, double variance, const uint32_t *key,
                                              double time_step, const uint8_t *positive_mask_host, float *log_likelihood,
                                              float *increments, float *ess, float *filtered_mean, float *filtered_std,
                                              float *particles, int *ancestors, float *log_weights, void *stream);
int vsde_residual_filter_replay(int kind, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0, const float *theta,
                                const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                const uint32_t *key, double time_step, const uint8_t *positive_mask_host, const float *particles,
                                const int *ancestors, const int *last_slot, float *paths, int *lineage, void *stream);
int vsde_crn_residual_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, int D, int T, const float *x0,
                                    const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                    double variance, const uint32_t *key, double time_step, const uint8_t *positive_mask_host,
                                    const float *particles, const int *ancestors, const int *last_slot, float *paths, int *lineage,
                                    void *stream);
int vsde_crn_kinetic_residual_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P, int K,
                                            int O, int D, int T, const float *x0, const float *rates, const int *obs_rows,
                                            const float *obs_values, const float *obs_matrix, double variance, const uint32_t *key,
                                            double time_step, const uint8_t *positive_mask_host, const float *particles,
                                            const int *ancestors, const int *last_slot, float *paths, int *lineage, void *stream);
int vsde_residual_anchored_replay(int kind, int B, int S, int P, int K, int O, int T, const float *x0, const float *theta,
                                  const int *obs_rows, const float *obs_values, const float *obs_matrix, double variance,
                                  const float *anchors, const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                  const uint8_t *positive_mask_host, float *paths, void *stream);
int vsde_crn_residual_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int O, int T, const float *x0,
                                      const float *theta, const int *obs_rows, const float *obs_values, const float *obs_matrix,
                                      double variance, const float *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                      double time_step, const uint8_t *positive_mask_host, float *paths, void *stream);
int vsde_crn_kinetic_residual_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K, int O,
                                              int T, const float *x0, const float *rates, const int *obs_rows, const float *obs_values,
                                              const float *obs_matrix, double variance, const float *anchors,
                                              const uint32_t *noise_path, const uint32_t *keys, double time_step,
                                              const uint8_t *positive_mask_host, float *paths, void *stream);

/* Exact simulation of the Markov jump process of a reaction network on integer copy numbers, the process whose diffusion
 * approximation the entry points above run (Gillespie's direct method; viforsdes_amd/core/jump_process.py is the specification).
 * B trajectories, a thread each: x0[B][S] (int32, 0 .. 2^30), theta[B][P] (P = R; the kinetic entry point takes rates[B][2R]),
 * out_times[K] (DEVICE float64, non-decreasing, >= 0), key: 2 words in DEVICE memory.  Propensity of reaction j at the state x:
 *   mass action  a_j = k_j prod_i x_i (x_i - 1) .. (x_i - r_ji + 1)   (falling factorial, in species order; no 1 / r!)
 *   rate law     the h_j of vsde_crn_kinetics with u = x_s, times 1[x_i >= r_ji for all i]
 * Event e (0-based) of path b: c_j = a_0 + .. + a_j in reaction order (fp32), a0 = c_{R-1}; a0 == 0: the state is absorbed and
 * fills every remaining output; else t += -log(u1) / a0 (the quotient in fp32, the clock t in float64), the reaction is the
 * smallest j with u2 a0 < c_j (none: the last j with a_j > 0), x += nu_j.  (u1, u2) are the uniforms ((w >> 8) + 0.5) 2^-24 of
 * words 2 (e & 1), 2 (e & 1) + 1 of philox4x32_10(counter {e >> 1, 0, b, 7}, key).  states[b][k] is the state after every event
 * with time <= out_times[k].
 *   status[b]: 0 complete; 1 the path fired max_events events before its last output time (outputs not reached: -1); 2 a
 * propensity was NaN, infinite or negative (outputs not reached: -1).  n_events[b]: the events fired.  E > 0: event_times[B][E]
 * (float64) and event_reactions[B][E] take the first E events of each path (NaN / -1 past the last); E = 0: both may be NULL.
 *   VSDE_E_BADARG before any HIP call: a bad descriptor (S, R, orders, rate laws) or one that disagrees with S / P; B or K < 1,
 * E < 0, max_events outside 1 .. 2^23 (with |nu| <= 127 and x0 <= 2^30 the int32 state cannot overflow), a NULL pointer, a NULL log
 * pointer with E > 0. */
int vsde_crn_jump_process(const vsde_crn_network *net, int B, int S, int P, int K, int E, const int32_t *x0, const float *theta,
                          const double *out_times, const uint32_t *key, int max_events, int32_t *states, int32_t *n_events,
                          int32_t *status, double *event_times, int32_t *event_reactions, void *stream);
int vsde_crn_kinetic_jump_process(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K, int E,
                                  const int32_t *x0, const float *rates, const double *out_times, const uint32_t *key,
                                  int max_events, int32_t *states, int32_t *n_events, int32_t *status, double *event_times,
                                  int32_t *event_reactions, void *stream);

/* Bootstrap particle filter whose particles are exact trajectories of the jump process above: log p^(y | theta) with no time step
 * and no diffusion approximation (viforsdes_amd/inference/jump_filter.py is the specification).  M filters, a workgroup each, N
 * particles (a multiple of 64; the limit depends on the network: 1024, and 512 for rate laws with more than 8 reactions), a
 * thread each: x0[M][S] (int32, 0 .. 2^30), theta[M][P] (the kinetic entry point: rates[M][2R]), obs_times[K] (DEVICE float64,
 * non-decreasing, >= 0), obs_values[K][O], obs_matrix[O][S] or NULL (O == S), key: 2 words in DEVICE memory.
 *   Segment k, from obs_times[k-1] (0 for k = 0) to obs_times[k], of particle slot j of filter m (path b = m N + j): the float64
 * clock restarts at exactly obs_times[k-1] and the event counter at 0; event e is the event of vsde_crn_jump_process on the
 * uniforms of philox4x32_10(counter {e >> 1, k, b, 7}, key) (the jump process is segment 0 of this stream); the segment ends as
 * soon as obs_times[k] < t + tau.  A particle that meets a NaN, infinite or negative propensity, or has fired max_events events
 * (counted per particle and per segment) short of obs_times[k], is stopped: it keeps its state, its log-weight at k is -inf, and
 * it carries on from that state only if the whole filter is dead.
 *   Observation k: lik_kind VSDE_LIK_GAUSSIAN (variance), VSDE_LIK_POISSON or VSDE_LIK_NEGATIVE_BINOMIAL (scale, dispersion,
 * row_const[K] as in vsde_count_particle_filter) on the state converted to fp32; NaN counts as -inf; then increments, ESS,
 * weighted moments before resampling, and systematic resampling, all by the rules of vsde_particle_filter (a dead filter: ancestors
 * = identity, increment -inf, ESS 0, moments NaN).  stopped[M][K] counts the stopped particles of segment k, mean_events[M][K]
 * the events per particle.  Optional outputs (NULL: not written): particles[M][K][N][S] (int32, before resampling),
 * ancestors[M][K][N], log_weights[M][K][N], events[M][K][N] (int32).
 *   VSDE_E_BADARG before any HIP call: a bad descriptor or one that disagrees with S / P; M or K < 1, N not a multiple of 64 or
 * above the network's limit, M N >= 2^32, O outside 1..16, O != S without obs_matrix, max_events outside 1 .. 2^23, an unknown
 * lik_kind, a variance / scale / dispersion <= 0, a NULL pointer among the required ones. */
#define VSDE_LIK_GAUSSIAN 0
int vsde_crn_jump_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const int32_t *x0,
                                  const float *theta, const double *obs_times, const float *obs_values, const float *obs_matrix,
                                  int lik_kind, double variance, double scale, double dispersion, const float *row_const,
                                  const uint32_t *key, int max_events, float *log_likelihood, float *increments, float *ess,
                                  float *filtered_mean, float *filtered_std, int32_t *stopped, float *mean_events,
                                  int32_t *particles, int *ancestors, float *log_weights, int32_t *events, void *stream);
int vsde_crn_kinetic_jump_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P, int K,
                                          int O, const int32_t *x0, const float *rates, const double *obs_times,
                                          const float *obs_values, const float *obs_matrix, int lik_kind, double variance,
                                          double scale, double dispersion, const float *row_const, const uint32_t *key,
                                          int max_events, float *log_likelihood, float *increments, float *ess, float *filtered_mean,
                                          float *filtered_std, int32_t *stopped, float *mean_events, int32_t *particles,
                                          int *ancestors, float *log_weights, int32_t *events, void *stream);

/* Replay of jump-process segments read at output times inside them: the latent paths of the jump-process particle smoother
 * (viforsdes_amd/inference/jump_smoother.py) and of particle MCMC with dynamics="jump".  B records by K segments, a thread per
 * (segment k, record r), k slowest.  Segment k of a record runs the event of vsde_crn_jump_particle_filter from its start state on
 * the uniforms of philox4x32_10(counter {e >> 1, k, b, 7}, key) for its path b, the float64 clock restarted at obs_times[k-1] (0 for
 * k = 0) and the event counter at 0, until obs_times[k] < t + tau.  path_times[Q] (DEVICE float64, non-decreasing, within
 * 0 .. obs_times[K-1]); q_begin[K+1] (DEVICE int32, q_begin[0] = 0, q_begin[K] = Q, non-decreasing; the caller's to get right,
 * the kernel clamps it into 0 .. Q): segment k owns the outputs q_begin[k] .. q_begin[k+1] - 1, the t_q with obs_times[k-1] < t_q <=
 * obs_times[k] (segment 0: from 0).  An output receives the state after every event with time <= t_q; a segment stopped by an
 * invalid propensity (status 2) or by max_events events short of obs_times[k] (status 1) leaves -1 in the outputs it did not reach.
 * Outputs: paths[B][Q][S] (int32), n_events[B][K], status[B][K].
 *   filter replay (the smoother): a record is (filter m, draw d), B = M D; x0[M][S], theta[M][P] (kinetic: rates[M][2R]), key: 2
 * words in DEVICE memory; particles[M][K][N][S] and ancestors[M][K][N] as the filter stored them; last_slot[M][D]: the slot of the
 * draw at the last observation (outside 0 .. N-1: a dead filter: lineage -1, paths -1, n_events 0, status 0).  The thread traces
 * its slots down to k and k - 1 (every entry clamped into 0 .. N-1), writes lineage[M][D][K], starts from x0[m] (k = 0) or
 * particles[m][k-1][lineage[k-1]] and uses path b = m N + lineage[k].
 *   anchored replay (PMMH): a record brings x0[B][S], theta[B][P], keys[B][2], anchors[B][K][S] (int32) and noise_path[B][K];
 * segment k starts at anchors[k-1] (x0 for k = 0) on path noise_path[k]; noise_path[K-1] = 0xFFFFFFFF: a dead record, as above.
 *   VSDE_E_BADARG before any HIP call: a bad descriptor or one that disagrees with S / P; M (B) or K < 1, N or D < 1, M N >= 2^32,
 * B K >= 2^31, Q < 1, max_events outside 1 .. 2^23, a NULL pointer. */
int vsde_crn_jump_filter_replay(const vsde_crn_network *net, int M, int N, int S, int P, int K, int D, int Q, const int32_t *x0,
                                const float *theta, const double *obs_times, const double *path_times, const int *q_begin,
                                const uint32_t *key, int max_events, const int32_t *particles, const int *ancestors,
                                const int *last_slot, int32_t *paths, int *lineage, int32_t *n_events, int32_t *status, void *stream);
int vsde_crn_kinetic_jump_filter_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P, int K,
                                        int D, int Q, const int32_t *x0, const float *rates, const double *obs_times,
                                        const double *path_times, const int *q_begin, const uint32_t *key, int max_events,
                                        const int32_t *particles, const int *ancestors, const int *last_slot, int32_t *paths,
                                        int *lineage, int32_t *n_events, int32_t *status, void *stream);
int vsde_crn_jump_anchored_replay(const vsde_crn_network *net, int B, int S, int P, int K, int Q, const int32_t *x0, const float *theta,
                                  const double *obs_times, const double *path_times, const int *q_begin, const int32_t *anchors,
                                  const uint32_t *noise_path, const uint32_t *keys, int max_events, int32_t *paths, int32_t *n_events,
                                  int32_t *status, void *stream);
int vsde_crn_kinetic_jump_anchored_replay(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K, int Q,
                                          const int32_t *x0, const float *rates, const double *obs_times, const double *path_times,
                                          const int *q_begin, const int32_t *anchors, const uint32_t *noise_path, const uint32_t *keys,
                                          int max_events, int32_t *paths, int32_t *n_events, int32_t *status, void *stream);

/* Tau-leaping for the jump process above: a fixed step tau = time_step with Poisson-many firings of every reaction on the integer
 * state (viforsdes_amd/core/tau_leap.py is the specification).  B trajectories, a thread each: x0[B][S] (int32, 0 .. 2^30),
 * theta[B][P] (P = R; the kinetic entry point takes rates[B][2R]), out_rows[K] (DEVICE int32, non-decreasing, >= 0: row r is read
 * after the steps 0 .. r - 1), key: 2 words in DEVICE memory.
 *   Step t of path b from the state x: a_j = the propensity of vsde_crn_jump_process (fp32); lam_j = a_j * (float)time_step, one
 * fp32 product, then widened to float64; n_j = the Poisson draw below for every j, all on the propensities at the start of the
 * step; then in reaction order on the running state (int64): n_j <- min(n_j, min over the species i with r_ji > 0 of floor(x_i /
 * r_ji)), x <- x + n_j nu_j; a reduced n_j adds 1 to capped[b].  The path stops with status 2 at a NaN, infinite or negative a_j,
 * a lam_j > 2^30, a failed draw, or an x_i > 2^30 after the last reaction of the step; it keeps the state from before that step,
 * the step adds nothing to capped[b], and the rows it has not reached hold -1.  status 0: complete.
 *   The draw, entirely in float64.  lam == 0: 0, no words read.  lam < 10: inversion on u1 of attempt 0: p = F = exp(-lam), n = 0;
 * while u1 > F and n < 63: n += 1, p = p (lam / n), F = F + p.  lam >= 10: Hoermann's PTRS (1993): b = 0.931 + 2.53 sqrt(lam), a =
 * -0.059 + 0.02483 b, 1/alpha = 1.1239 + 1.1328 / (b - 3.4), v_r = 0.9277 - 3.6224 / (b - 2); attempt q: Uc = u1 - 0.5, V = u2,
 * us = 0.5 - |Uc|; reject if us < 0.013 and V > us; n = floor(((2 a) / us + b) Uc + lam + 0.43); accept if us >= 0.07 and V <=
 * v_r; reject if n < 0; accept if (log V + log(1/alpha)) - log(a / (us us) + b) <= (-lam + n log lam) - lgamma(n + 1); the draw
 * fails after 32 attempts.  Attempt q of reaction j at step t reads w = philox4x32_10(counter {t, j | ((q >> 1) << 16), b, 8},
 * key): u1, u2 = the uniforms ((w >> 8) + 0.5) 2^-24 (fp32) of words 2 (q & 1), 2 (q & 1) + 1.
 *   E > 0: draws[B][E][R] takes the raw draws (before the cap) of steps 0 .. E - 1, -1 from the step the path stopped at (or never
 * took) on; E = 0: draws may be NULL.
 *   VSDE_E_BADARG before any HIP call: a bad descriptor or one that disagrees with S / P; B or K < 1, E < 0, a time_step that is
 * not positive and finite, a NULL pointer, a NULL draws with E > 0. */
int vsde_crn_tau_leap_process(const vsde_crn_network *net, int B, int S, int P, int K, int E, const int32_t *x0, const float *theta,
                              const int32_t *out_rows, const uint32_t *key, double time_step, int32_t *states, int32_t *status,
                              int32_t *capped, int32_t *draws, void *stream);
int vsde_crn_kinetic_tau_leap_process(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int B, int S, int P, int K, int E,
                                      const int32_t *x0, const float *rates, const int32_t *out_rows, const uint32_t *key,
                                      double time_step, int32_t *states, int32_t *status, int32_t *capped, int32_t *draws,
                                      void *stream);

/* Bootstrap particle filter whose particles are tau-leap trajectories (viforsdes_amd/inference/tau_leap_filter.py is the
 * specification).  M filters, a workgroup each, N particles (a multiple of 64 up to 512: the float64 sampler needs more registers
 * than a 1024-thread workgroup leaves a lane), a thread each: x0[M][S] (int32, 0 .. 2^30), theta[M][P] (the kinetic entry point:
 * rates[M][2R]), obs_rows[K] (DEVICE int32, non-decreasing, >= 0), obs_values[K][O], obs_matrix[O][S] or NULL (O == S), key: 2
 * words in DEVICE memory.
 *   Segment k runs the steps obs_rows[k-1] .. obs_rows[k] - 1 (obs_rows[-1] = 0) of vsde_crn_tau_leap_process for particle slot j
 * of filter m as path b = m N + j: a slot keeps its stream across resampling, and the tau-leap process is segment 0.  A stopped
 * particle keeps its state, its log-weight at k is -inf, and it carries on from that state only if the whole filter is dead.
 *   Observation k, the outputs log_likelihood[M], increments, ess [M][K], filtered_mean, filtered_std [M][K][S] and the optional
 * particles[M][K][N][S] (int32, before resampling), ancestors[M][K][N], log_weights[M][K][N] are those of
 * vsde_crn_jump_particle_filter.  stopped[M][K] counts the stopped particles of segment k, capped[M][K] the reduced draws of its
 * particles (summed in fp32: exact up to 2^24).
 *   VSDE_E_BADARG before any HIP call: as vsde_crn_jump_particle_filter, with time_step (positive, finite) in place of
 * max_events. */
int vsde_crn_tau_leap_particle_filter(const vsde_crn_network *net, int M, int N, int S, int P, int K, int O, const int32_t *x0,
                                      const float *theta, const int32_t *obs_rows, const float *obs_values, const float *obs_matrix,
                                      int lik_kind, double variance, double scale, double dispersion, const float *row_const,
                                      const uint32_t *key, double time_step, float *log_likelihood, float *increments, float *ess,
                                      float *filtered_mean, float *filtered_std, int32_t *stopped, int32_t *capped,
                                      int32_t *particles, int *ancestors, float *log_weights, void *stream);
int vsde_crn_kinetic_tau_leap_particle_filter(const vsde_crn_network *net, const vsde_crn_kinetics *kin, int M, int N, int S, int P,
                                              int K, int O, const int32_t *x0, const float *rates, const int32_t *obs_rows,
                                              const float *obs_values, const float *obs_matrix, int lik_kind, double variance,
                                              double scale, double dispersion, const float *row_const, const uint32_t *key,
                                              double time_step, float *log_likelihood, float *increments, float *ess,
                                              float *filtered_mean, float *filtered_std, int32_t *stopped, int32_t *capped,
                                              int32_t *particles, int *ancestors, float *log_weights, void *stream);

/* Measurement aid (no reference counterpart): when enabled, the launchers bracket their kernels with hipEvents on the
 * launch stream.  which: 0 = serial time-stepping forward kernel (training variant), 1 = serial backward kernel,
 * 2 = everything vsde_head_forward enqueues (training variant), 3 = everything vsde_head_backward enqueues,
 * 4 = the forward's context-projection GEMM, 5 = the backward's grad_context GEMM, 6 = the grouped weight-gradient
 * reduction.  vsde_profile_elapsed_ms waits for the end event of the LAST such launch. */
int vsde_profile_enable(int on);
/* Test hook: route L <= 2 through the LDS-resident one-wave-per-path kernels that serve L = 3, 4. */
int vsde_debug_force_v1(int on);
/* Which forward time-stepping kernel serves hidden_dim 64 / L <= 2 / state_dim <= 2 (reference kernels/forward.py:137-375):
 * mode 1 = the multi-path MFMA kernel (16 paths per workgroup, csrc/vsde_head_mp.hip) whenever applicable, 0 = never (the
 * four-waves-per-path kernel), < 0 = default (environment VSDE_HEAD_MP, else by batch size). */
int vsde_debug_head_mp(int mode);
/* 1 once a GRU head weight has left the f16 range of the multi-path MFMA kernels (|W| > 2.2e4; the weight preparation of every such
 * launch checks): the launch that found it returns NON-FINITE paths (never silently wrong ones), and every later launch of the process
 * takes the fp32 four-waves-per-path kernels.  The flag lives in host-mapped memory and is written in stream order: a caller that
 * REPLAYS a captured graph (whose kernel choice was fixed at capture) polls it after a replay and re-captures / steps eagerly.
 * mode > 0 clears the flag (tests).  No reference counterpart (the reference's Triton kernels are fp32 throughout). */
int vsde_head_mfma_range_exceeded(int clear);
int vsde_profile_elapsed_ms(int which, float *ms);

/* Test hooks: the non-recurrent GEMM stages of the head alone, on operands the caller supplies (no reference counterpart).  Both run
 * the host code the product entry points run -- the weight packing and the same dispatch -- and nothing of the time loop; all
 * argument checks come before the first HIP call.  `w` is the head's full weight set (the packing kernel reads every matrix).
 *   context projection: G[B*T][3H] (fp32, contiguous) = ctx W_ih_l0[:, S:S+C]^T + b_ih_l0; workspace as for vsde_head_forward.
 *   backward GEMMs: from the pre-activation gradients D4[B][T][L][4][H] (slots dr, du, dn, dc_n), the emission gradients
 *   DO[B][T][S + S(S+1)/2], paths[B][T+1][S] and acts[B][T][L][5][H] it writes grads->context (context_dtype /
 *   context_batch_stride as in vsde_head_backward) and the ten weight / bias gradients; grads->x0 and grads->theta are not touched.
 *   Workspace as for vsde_head_backward. */
int vsde_debug_head_context_projection(const vsde_head_dims *d, const vsde_context_view *ctx, const vsde_head_weights *w,
                                       float *G, void *workspace, size_t workspace_bytes, void *stream);
int vsde_debug_head_backward_gemms(const vsde_head_dims *d, const vsde_context_view *ctx, const float *theta,
                                   const float *paths, const float *acts, const float *D4, const float *DO,
                                   const vsde_head_weights *w, const vsde_head_grads *grads, void *workspace,
                                   size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* VSDE_HIP_H */
