/*
 * slode.h -- C ABI of libslode.so: the MI355X (gfx950) engine for the latent-ODE solve + ELBO path of
 * paidamoyo/structured_latent_ODEs.
 *
 * The reference has no FFI of its own (its only API is Python classes); every entry point below
 * names the reference Python interface it replaces (file:line relative to the reference repo).  The Python host
 * side (structured_latent_odes_amd/) binds these with ctypes; INTEGRATION.md shows the stub a reference
 * maintainer would add.
 *
 * Conventions
 *   - all tensors are fp32, device (HBM) pointers owned by the CALLER; the library never allocates device
 *     memory, never synchronises the stream, and launches on the hipStream_t passed as `void* stream`;
 *   - the environment is read once per handle, in slode_create (diagnostic switches SLODE_NO_FOLD, SLODE_ODE_LOOP, SLODE_ODE_GRID,
 *     SLODE_ODE_GENERIC, SLODE_ODE_ALG, SLODE_ODE_PACK, SLODE_ENC_FUSE, SLODE_DP5_LPT); nothing about a launch depends on the environment at call time;
 *   - `times` must be strictly monotone (torchdiffeq's precondition); a table that is not turns the fused kernel's loss into NaN;
 *   - every call returns SLODE_OK (0) or a negative slode_status; slode_last_error() gives the text;
 *   - all model parameters live in ONE flat fp32 vector whose segment offsets are given by slode_layout
 *     (filled by slode_layout_init); gradients use the same layout;
 *   - observations are addressed as the logical [B, C, T] tensor through explicit element strides, so the
 *     reference's permuted view of a contiguous [B, T, C] batch (training_cvs.py:25) is consumed without a copy.
 */
#ifndef SLODE_H
#define SLODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLODE_VERSION 290 /* 0.2.9: slode_pointwise_loo, slode_loo_plan; slode_intervene_summary, slode_intervene_summary_plan; slode_forecast_summary, slode_forecast_summary_plan (additions to 0.2.9: no entry point or struct of 0.2.9 changes, so the number stands) (0.2.8: slode_joint_band, slode_joint_band_plan, slode_joint_band_levels; 0.2.7: slode_mechanism_moments, slode_mechanism_plan; 0.2.6: slode_recon_quantiles, slode_quantile_plan; 0.2.5: slode_curve_summary, slode_curve_summary_plan; 0.2.4: slode_latent_attribution, slode_attribution_plan; 0.2.3: slode_pointwise_density, slode_pointwise_plan; 0.2.2: slode_posterior_refine; 0.2.1: slode_label_evidence; 0.2.0: slode_calibration, slode_calibration_plan; 0.1.9: slode_cohort_moments, slode_cohort_plan; 0.1.8: slode_forecast_moments, slode_forecast_plan, slode_stage_times_n; 0.1.7: slode_intervene_moments; 0.1.6: slode_traj_bounds; 0.1.5: slode_recon_moments; 0.1.4: slode_eval_stats; 0.1.3: slode_shape::particles; 0.1.2: SLODE_BOSH3, SLODE_FEHLBERG2, SLODE_ADAPTIVE_HEUN; 0.1.1: slode_svi_step, slode_rng_*, slode_grad_*) */

#define SLODE_MAX_GROUPS 4
#define SLODE_MAX_HEADS 3
#define SLODE_MAX_AUX 4
#define SLODE_MAX_LABELS 4 /* label tensors of one minibatch (proc: aR, aS, C12, C6) */
#define SLODE_MAX_PARTICLES 1024
#define SLODE_EVAL_SLOTS 8 /* floats of one slode_eval_stats row */
#define SLODE_BOUND_SLOTS 4 /* floats of one slode_traj_bounds row */
#define SLODE_EVIDENCE_SLOTS 4 /* floats of one (trajectory, hypothesis) row of slode_label_evidence */
#define SLODE_EVIDENCE_MAX_V 64 /* most hypotheses of one slode_label_evidence call */
#define SLODE_COHORT_MAX_G 1024 /* most cohorts of one slode_cohort_moments call */
#define SLODE_COHORT_MAX_CHUNK 64 /* most members one workgroup folds into one partial */
#define SLODE_CALIBRATION_PHI2 0.97724986805182079f  /* Phi(2): the nominal level of mean + 2 s */
#define SLODE_CALIBRATION_PHIM2 0.022750131948179195f /* Phi(-2): of mean - 2 s */
#define SLODE_ATTRIBUTION_MAX_ARMS 16 /* most arms (block masks) of one slode_latent_attribution call */
#define SLODE_SUMMARY_SLOTS 8 /* functionals of one slode_curve_summary row: peak, t_peak, trough, t_trough, auc, time_beyond, t_hit, crossed */
#define SLODE_INTERVENE_SUMMARY_MAX_ARMS 64 /* most hypotheses (counterfactual arms) of one slode_intervene_summary call */
#define SLODE_QUANTILE_MAX_LEVELS 8 /* most levels of one slode_recon_quantiles call */
#define SLODE_JOINT_BAND_MAX_LEVELS 8 /* most levels of one slode_joint_band call */
#define SLODE_MECHANISM_SLOTS 5 /* slots of slode_mechanism_moments: state, production, degradation, set_point, net_rate */
#define SLODE_FORECAST_MAX_T (1 << 20) /* most points of an output grid (slode_stage_times_n, slode_forecast_moments) */

typedef enum slode_status {
  SLODE_OK = 0,
  SLODE_EINVAL = -1, /* bad shape / stride / null pointer / unsupported dimension */
  SLODE_EHIP = -2,   /* a HIP runtime call failed (text from hipGetErrorString)      */
  SLODE_ENOSPC = -3  /* caller workspace too small                                   */
} slode_status;

/* torchdiffeq method strings accepted by OdeModel.init_with_params(solver=...), models/blackbox_ode.py:7-17,41-45 */
typedef enum slode_method {
  SLODE_EULER = 0, SLODE_MIDPOINT = 1, SLODE_RK4 = 2,   /* fixed grid */
  SLODE_DOPRI5 = 3, SLODE_BOSH3 = 4, SLODE_FEHLBERG2 = 5, SLODE_ADAPTIVE_HEUN = 6   /* adaptive (see slode_elbo_step) */
} slode_method;

/* Decoder (models/decoders.py:8-54, asymmetric-Laplace, 3 heads q50/q75/q25) or GaussianDecoder (:57-91, 1 head) */
typedef enum slode_likelihood { SLODE_ALD = 0, SLODE_GAUSS = 1 } slode_likelihood;
/* SLODE_GRAD_EXACT: exact gradient of the discrete scheme (== reference with adjoint_solver=False).
 * SLODE_GRAD_REFERENCE_ADJOINT: what torchdiffeq.odeint_adjoint returns, the reference default (models/blackbox_ode.py:40-42,
 * adjoint_solver = True in all three configs): the continuous adjoint stepped backwards with the same fixed-grid method, and NO
 * gradient to z through the dynamics (OdeFunc.constants is not a parameter, :55).  Fixed-grid methods, ELBO / solve backward. */
typedef enum slode_grad_mode { SLODE_GRAD_EXACT = 0, SLODE_GRAD_REFERENCE_ADJOINT = 1 } slode_grad_mode;

/* One conditional prior net p(z_g | u_g): EncoderMLP([u_dim, [z_dim, z_dim]], [None, Exp]);
 * models/mechanistic_cvs.py:88-100, mechanistic_proc.py:107-114, mechanistic_challenge.py:88-95 */
typedef struct slode_group {
  int32_t z_off, z_dim; /* latent dims [z_off, z_off + z_dim) */
  int32_t u_off, u_dim; /* label columns [u_off, u_off + u_dim) of u[B, n_u] */
} slode_group;

/* A label head q(label | z_g): EncoderMLP([z_dim, U, u_dim]) with one Softplus hidden layer.  Scored at `aux_mult` x by the
 * auxiliary loss (model_meta: mechanistic_cvs.py:240-270, mechanistic_proc.py:313-353, mechanistic_challenge.py:264-291) and,
 * when `aux_in_main` is set (the proc family: q_label / q_continous on the replayed z, mechanistic_proc.py:145-146), also
 * inside the main loss.
 *   SLODE_AUX_SIGMOID: Bernoulli(probs = sigmoid(.));  SLODE_AUX_SOFTMAX: OneHotCategorical(probs = softmax(.));
 *   SLODE_AUX_EXPEXP:  two Exp heads [loc, unused], Laplace(loc, softplus(constant_std_*)) on the label. */
typedef enum slode_aux_kind { SLODE_AUX_SIGMOID = 0, SLODE_AUX_SOFTMAX = 1, SLODE_AUX_EXPEXP = 2 } slode_aux_kind;
typedef struct slode_aux {
  int32_t kind;
  int32_t z_off, z_dim; /* latent dims the head reads */
  int32_t u_off, u_dim; /* label columns it scores   */
} slode_aux;

typedef struct slode_shape {
  int32_t B;  /* trajectories in this call (per GPU)                                   */
  int32_t T;  /* time points (len(times))                                              */
  int32_t C;  /* observed channels, config.obs_dim                                      */
  int32_t L;  /* latent dim = sum of z_*_dim                                           */
  int32_t S;  /* config.ode_state_dim                                                  */
  int32_t H;  /* config.ode_hidden_dim                                                 */
  int32_t F;  /* config.n_filters                                                      */
  int32_t K;  /* config.filter_size                                                    */
  int32_t P;  /* config.pool_size                                                      */
  int32_t Hc; /* config.cnn_hidden_dim                                                 */
  int32_t n_u;      /* label columns of u                                              */
  int32_t n_groups; /* conditional prior groups; remaining latent dims are N(0, 1)     */
  slode_group groups[SLODE_MAX_GROUPS];
  int32_t method;     /* slode_method                                                  */
  int32_t likelihood; /* slode_likelihood                                              */
  float quantile_diff; /* config.quantile_diff (ALD only), data/cvs/config_cvs.py:48    */
  float rtol, atol;    /* adaptive methods (torchdiffeq defaults 1e-7 / 1e-9)           */
  int32_t n_aux;       /* label heads (auxiliary loss; also the main loss iff aux_in_main)  */
  int32_t U;           /* config.u_hidden_dim (<= 32)                                      */
  float aux_mult;      /* config.aux_loss_multiplier                                       */
  slode_aux aux[SLODE_MAX_AUX];
  int32_t aux_in_main; /* 1: the main model scores the label heads too (proc family)       */
  int32_t grad_mode;   /* slode_grad_mode: which gradient the backward pass returns         */
  /* pyro.infer.Trace_ELBO(num_particles=K) (training_cvs.py:237 `Trace_ELBO(num_particles=config.num_particles)`): the ELBO steps
   * (slode_elbo_step, slode_elbo_adam_step, slode_aux_step, slode_svi_step, slode_grad_partial / slode_grad_apply; kind MAIN and AUX)
   * evaluate model and guide K times on the same minibatch and parameters, each with its own reparameterisation noise, and return the
   * MEAN of the K losses and the MEAN of the K gradients; Adam, where the step applies it, steps ONCE with that mean.  0 and 1 both mean
   * one particle (a zero-initialised shape behaves as before this field existed); at most SLODE_MAX_PARTICLES.  The encoder runs once
   * (its output does not depend on the particle); the solver / scorer kernels run over K * B virtual trajectories, particle-major:
   * virtual row k * B + b is particle k of data row b.
   *   Noise: eps == NULL draws particle k from drawing call n + k of the handle's generator (n = the counter at the call; trajectory
   *   index unchanged, so sharding stays a matter of first_trajectory alone) and leaves the counter at n + K:
   *   slode_rng_normal(h, n + k, B, L, ...) reads particle k's noise back.  eps != NULL is one dense [K, B, L] tensor ([B, L] for K = 1).
   *   Limits are the per-call ones applied to B * K: the adaptive methods' 65,536 trajectories (SLODE_EINVAL beyond), their step-record
   *   capacity 2^26 / (B K (S + 2)) clamped to [64, 2048]; slode_dopri5_step_counts returns K * B counts (virtual-row order).
   *   x_out / z_out with K > 1: SLODE_EINVAL.  A handle created with SLODE_FOLD_NEXT, SLODE_ODE_PACK or SLODE_ODE_ALG set refuses K > 1
   *   (SLODE_EINVAL): the measured arms take one particle.  slode_workspace_bytes accounts for K.  The other entry points ignore it. */
  int32_t particles;
} slode_shape;

/* Offsets (in floats) of each parameter tensor inside the flat parameter / gradient vector.
 * Names are the reference state_dict keys they hold. */
typedef struct slode_layout {
  int32_t conv_w, conv_b;   /* encoder.conv.{weight[F,C,K], bias[F]}          encoder_conv.py:31 */
  int32_t lin_w, lin_b;     /* encoder.lin.{weight[Hc,F*n_pool], bias[Hc]}    encoder_conv.py:34 */
  int32_t zloc_w, zloc_b;   /* encoder.z_loc.{weight[L,Hc], bias[L]}          encoder_conv.py:37 */
  int32_t zls_w, zls_b;     /* encoder.z_scale.0.{weight[L,Hc], bias[L]}      encoder_conv.py:38 */
  int32_t ode_begin;        /* start of the segment the fused ODE/ELBO kernel differentiates      */
  int32_t ploc_w[SLODE_MAX_GROUPS], ploc_b[SLODE_MAX_GROUPS]; /* <prior>.sequential_mlp.1.0.0.*      */
  int32_t pls_w[SLODE_MAX_GROUPS], pls_b[SLODE_MAX_GROUPS];   /* <prior>.sequential_mlp.1.1.0.*      */
  int32_t init_w1, init_b1; /* decoder.ode_model.latent_to_ode_net.0.{weight[H,L], bias[H]}          */
  int32_t init_w2, init_b2; /* decoder.ode_model.latent_to_ode_net.2.{weight[S,H], bias[S]}          */
  int32_t dyn_wh, dyn_bh;   /* ...dynamics.dynamics_hidden.{weight[H,1+L], bias[H]} (col 0 = time)   */
  int32_t dyn_wg, dyn_bg;   /* ...dynamics.dyanamics_growth.{weight[S,H], bias[S]}                   */
  int32_t dyn_wd, dyn_bd;   /* ...dynamics.dyanmics_degradation.{weight[S,H], bias[S]}               */
  int32_t head_w[SLODE_MAX_HEADS]; /* decoder.output_{q50,q75,q25}.0.weight[C,S] | output_mean (Gauss) */
  /* label heads of the main loss: <head>.sequential_mlp.1.module.{weight[U,z_dim],bias[U]}, .3.{weight[u_dim,U],bias}
   * (EXPEXP: .3.0.0.* then .3.1.0.*), and for EXPEXP the scalar constant_std_C_* */
  int32_t aux_w1[SLODE_MAX_AUX], aux_b1[SLODE_MAX_AUX], aux_w2[SLODE_MAX_AUX], aux_b2[SLODE_MAX_AUX];
  int32_t aux_w3[SLODE_MAX_AUX], aux_b3[SLODE_MAX_AUX], aux_c[SLODE_MAX_AUX];
  int32_t cstd;             /* decoder.constant_std[C,T]                                             */
  int32_t ode_end;          /* end of that segment                                                   */
  int32_t n_params;         /* total floats covered by this layout; callers may append their own      */
} slode_layout;

typedef struct slode_ctx* slode_handle;

int slode_version(void);
/* device_id >= 0: HIP device ordinal.  There is no CPU backend: a process without a gfx950 device gets SLODE_EHIP. */
int slode_create(slode_handle* h, int device_id);
int slode_destroy(slode_handle h);
const char* slode_last_error(slode_handle h); /* valid until the next call on h; h may be NULL (global text) */

/* Validates `s` (SLODE_EINVAL on unsupported dimensions) and fills the canonical layout. */
int slode_layout_init(const slode_shape* s, slode_layout* lay);
/* Number of stage times the fixed-grid method evaluates: R*(T-1)+1 (R = 1/2/3 for euler/midpoint/rk4). */
int slode_num_stage_times(const slode_shape* s);
/* Bytes of caller workspace needed by slode_elbo_step / the *_bwd ops for this shape. */
size_t slode_workspace_bytes(slode_handle h, const slode_shape* s);

/* Stage-time table: the distinct times at which the fixed-grid solver evaluates f, computed on device with the
 * same fp32 arithmetic as torchdiffeq's step functions (t0 + dt/3, ...).  Replaces the time bookkeeping inside
 * torchdiffeq.odeint for the call at models/blackbox_ode.py:41-45.  times[T] -> stage_t[slode_num_stage_times]. */
int slode_stage_times(slode_handle h, const slode_shape* s, const float* times, float* stage_t, void* stream);

/* EncoderCONV.forward (models/encoder_conv.py:43-51): obs (logical [B,C,T], strides in elements) -> loc, scale [B,L].
 * `pooled` [B, F*n_pool] and `hid` [B, Hc] are saved for the backward (either may be NULL for inference). */
int slode_encoder_conv_fwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                           const float* obs, const int64_t obs_strides[3], float* loc, float* scale,
                           float* pooled, float* hid, void* stream);

/* Backward of EncoderCONV.forward: (g_loc, g_scale) [B,L] -> grads[conv_w .. zls_b] (overwritten, not accumulated). */
int slode_encoder_conv_bwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                           const float* obs, const int64_t obs_strides[3], const float* scale,
                           const float* pooled, const float* hid, const float* g_loc, const float* g_scale,
                           float* grads, void* workspace, size_t workspace_bytes, void* stream);

/* OdeModel.solve_ODE (models/blackbox_ode.py:36-47): z[B,L] -> x[B,T,S] (contiguous; the reference returns the
 * same logical tensor as a permuted view).  stage_t from slode_stage_times. */
int slode_ode_solve_fwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                        const float* times, const float* stage_t, const float* z, float* x, void* stream);

/* Exact discrete adjoint of slode_ode_solve_fwd (== autograd through torchdiffeq.odeint, adjoint_solver=False):
 * g_x[B,T,S] -> g_z[B,L] and grads[init_w1 .. dyn_bd] (overwritten).
 * Of `params` the call reads the flat range [lay->ode_begin, lay->n_params) only -- nothing of the encoder below it -- so a caller may pass
 * (copy of that range) - lay->ode_begin as `params`: the weights of an earlier forward, frozen (the Python layer's autograd backward does). */
int slode_ode_solve_bwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                        const float* times, const float* stage_t, const float* z, const float* g_x,
                        float* g_z, float* grads, void* workspace, size_t workspace_bytes, void* stream);

/* OdeFunc.forward(t, state) (models/blackbox_ode.py:57-61 -> Dynamics.forward :97-109): one evaluation of
 * dx/dt = a(t,z) - d(t,z) * state for state[B,S], z[B,L] -> out[B,S].  API completeness; the solver does not use it. */
int slode_dynamics_eval(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, float t,
                        const float* state, const float* z, float* out, void* stream);

/* OdeModel.initialize_state (models/blackbox_ode.py:19-22, 32-34): z[B,L] -> x0[B,S] = sigmoid(W2 relu(W1 z + b1) + b2). */
int slode_initialize_state(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* z, float* x0,
                           void* stream);

/* The conditional prior nets p(z_g | u_g) (EncoderMLP([u_dim, [z_dim, z_dim]], [None, Exp]).forward; call sites
 * models/mechanistic_cvs.py:225-237, 304-311 (prior reconstructions)): u[B,n_u] -> loc, scale [B,L]; latent dims outside every group get
 * loc 0, scale 1 (the N(0,1) prior of z_epsilon). */
int slode_prior_nets(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* u, float* loc,
                     float* scale, void* stream);

/* The label heads q(label | z_g) (EncoderMLP([z_dim, U, u_dim]).forward; call sites: classifier / pred_inputs,
 * models/mechanistic_cvs.py:278-296, mechanistic_proc.py:361-380): z[B,L] -> out[B,n_u], every head writing the label columns it scores:
 * Bernoulli probabilities (SIGMOID), class probabilities (SOFTMAX) or the Laplace location exp(.) (EXPEXP). */
int slode_label_heads(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* z, float* out,
                      void* stream);

/* Decoder.forward / GaussianDecoder.forward heads (models/decoders.py:45-53, 86-89) on a given trajectory:
 * x[B,T,S] -> mu[Q][B,C,T] (Q = 3: mu_50, mu_75, mu_25 in that order; Q = 1: mean) and std[C,T] = softplus(constant_std). */
int slode_decode_heads(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                       const float* x, float* mu, float* std_ct, void* stream);

/* Backward of slode_decode_heads (autograd through Decoder.forward / GaussianDecoder.forward, models/decoders.py:42-54, 84-91, as the
 * reference's recon-style callers would differentiate it): g_mu[Q][B,C,T] (zeros for heads without a gradient), g_std[C,T] (NULL: none) ->
 * g_x[B,T,S], g_heads[Q][C,S] (the head weights' gradients, in slode_decode_heads' head order), g_cstd[C,T] (NULL to skip).
 * Of `params` the call reads the flat range [lay->head_w[0], lay->n_params) only (the head weights and constant_std), so a caller may pass
 * (copy of that range) - lay->head_w[0] as `params`. */
int slode_decode_heads_bwd(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* x,
                           const float* g_mu, const float* g_std, float* g_x, float* g_heads, float* g_cstd, void* stream);

/* One SVI step's arithmetic for the main loss (pyro SVI.step on (model, guide); call sites training_cvs.py:152,236;
 * models/mechanistic_cvs.py:105-238 and the proc/challenge equivalents):
 *   encoder -> z = loc + scale*eps -> log q, log p -> ODE solve -> heads -> ALD/Gauss likelihood -> -ELBO (summed
 *   over the batch) -> exact gradient wrt every parameter of the layout.
 * Outputs: loss_out[0] = -ELBO (float, device); grads[0 .. lay->n_params) overwritten.
 * With grads == NULL only the loss is computed (SVI.evaluate_loss, training_cvs.py:81).
 * Optional outputs (NULL to skip): x_out[B,T,S] latent trajectories, z_out[B,L].
 * method == SLODE_DOPRI5 (solver="dopri5", models/blackbox_ode.py:41-45): adaptive solve with one controller per trajectory
 * (rtol / atol of the shape); the gradient is the reverse mode of the accepted steps and of the dense output, step sizes held fixed
 * (grad_mode SLODE_GRAD_REFERENCE_ADJOINT: without the z -> dynamics path, as odeint_adjoint).  stage_t is ignored.  At most 65,536
 * trajectories per call; a trajectory whose accepted steps exceed the record capacity (256 MB / (B*(S+2)) floats, clamped to
 * [64, 2048] steps) or that exhausts 20,000 attempted steps turns the loss into NaN.  slode_workspace_bytes accounts for the records, for
 * the running sums the reverse sweep parks at the hidden units' switching times ([B][2][H][4S]: one set per lane group of a trajectory) and
 * for the forward kernel's set-up tables of every sixteen trajectories, which the reverse sweep reads back instead of rebuilding them.
 * method == SLODE_BOSH3 / SLODE_FEHLBERG2 / SLODE_ADAPTIVE_HEUN (torchdiffeq's other RKAdaptiveStepsizeODESolver methods: Bogacki-Shampine
 * 3(2), Fehlberg 2(1), Heun-Euler 2(1)): the same contract as dopri5 -- one controller per trajectory, rtol / atol of the shape, a step
 * at the fp32 time floor accepted, 20,000 attempts, the same record of accepted steps with the same capacity, the same overflow and
 * failed-solve results, the reverse mode of the method's own stages and dense output -- with the method's tableau and its order p in
 * the controller (factor 0.9 ratio^(-1/p)) and in the Hairer initial step ((0.01 / max(d1, d2))^(1/p)).  The low orders take many more
 * steps at the same tolerance (measured at cvs B = 1024 T = 200 and config[2] B = 4096 T = 100): bosh3 and fehlberg2 train at
 * both shapes at the defaults (bosh3 141-428 accepted steps, fehlberg2 225-751); adaptive_heun trains down to rtol 1e-5 / atol 1e-7
 * (356-1206 steps) and at the defaults (3516-11906 steps) overflows the record, and the step returns NaN by contract.
 * Forward-only solves (slode_ode_solve_fwd) take every adaptive method.  SLODE_DP5_LPT=32 / 64 (a test hook) is dopri5-only: with
 * another adaptive method the step returns SLODE_EINVAL. */
int slode_elbo_step(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params,
                    const float* times, const float* stage_t, const float* obs, const int64_t obs_strides[3],
                    const float* u, const float* eps, float* loss_out, float* grads, float* x_out, float* z_out,
                    void* workspace, size_t workspace_bytes, void* stream);

/* slode_elbo_step immediately followed by slode_adam_step, with the Adam update applied by the final gradient-reduction
 * kernel (one launch and one pass over the gradient less; identical arithmetic).  For single-process training: data-parallel
 * runs need the gradient materialised for the all-reduce between the two, so they call the two entry points separately.
 * params / exp_avg / exp_avg_sq hold n_total >= lay->n_params floats; entries beyond the layout (caller-appended parameters the
 * main loss does not touch) are stepped with a zero gradient, as pyro's shared optimizer does.  grads is still
 * written ([0, n_params)). */
int slode_elbo_adam_step(slode_handle h, const slode_shape* s, const slode_layout* lay, float* params, const float* times,
                         const float* stage_t, const float* obs, const int64_t obs_strides[3], const float* u, const float* eps,
                         float* loss_out, float* grads, void* workspace, size_t workspace_bytes, int64_t n_total, float* exp_avg,
                         float* exp_avg_sq, float lr, float beta1, float beta2, float adam_eps, int64_t step, void* stream);

/* One step of the reference's SECOND SVI object, SVI(model_meta, guide_meta) (training_cvs.py:244-249,152): encoder ->
 * group latents z_g = loc_g + scale_g * eps_g sampled in the model -> -[sum log N(z_g; loc_g, scale_g) + aux_mult * sum_heads
 * log p(label | head(z_g))], summed over the batch, and its exact gradient (encoder and label-head parameters; every other
 * entry of grads[0, n_params) is written as 0).  grads == NULL: loss only (evaluate_loss).  If exp_avg != NULL the Adam update
 * of all n_total >= n_params parameters is applied by the final reduction kernel (as slode_elbo_adam_step). */
int slode_aux_step(slode_handle h, const slode_shape* s, const slode_layout* lay, float* params, const float* obs,
                   const int64_t obs_strides[3], const float* u, const float* eps, float* loss_out, float* grads, void* workspace,
                   size_t workspace_bytes, int64_t n_total, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2,
                   float adam_eps, int64_t step, void* stream);

/* ---- one SVI.step(**batch) as ONE call (training_cvs.py:147-157: `losses[i].step(**d)`) ------------------------------------------------
 * The minibatch as the reference's loader and batch_to_device hand it over (training_cvs.py:18-27, training_proc.py:25-33,
 * training_challenge.py:27-33): the observation tensor with its strides and the label tensors ONE BY ONE -- dense [B, width] each, in the
 * order in which the model concatenates them into u (cvs: iext, rtpr; proc: aR, aS, C12, C6; challenge: symptoms, shedding) -- no host-side
 * concatenation.  eps == NULL: the reparameterisation noise of the guide's sample sites (mechanistic_cvs.py:225-237 `pyro.sample(...,
 * dist.Normal(loc, scale).to_event(1))`; model_meta :256-262 for the auxiliary loss) is drawn INSIDE the kernels from the handle's
 * counter-based generator (slode_rng_seed); eps != NULL ([B, L], the explicit-noise parity path) is used as is. */
typedef struct slode_batch {
  const float* obs;            /* logical [B, C, T] */
  int64_t obs_strides[3];      /* element strides */
  int32_t n_labels;            /* 0: no labels (shapes without conditional priors / label heads) */
  int32_t label_width[SLODE_MAX_LABELS];
  const float* labels[SLODE_MAX_LABELS];
  const float* eps;            /* [B, L] ([K, B, L] with the shape's particles = K > 1) or NULL */
} slode_batch;
/* Adam hyper-parameters and state for the update applied by the step's last kernel (NULL: gradient only) */
typedef struct slode_adam {
  int64_t n_total;             /* floats in params / exp_avg / exp_avg_sq (>= lay->n_params) */
  float *exp_avg, *exp_avg_sq;
  float lr, beta1, beta2, eps;
  int64_t step;                /* 1-based */
} slode_adam;
typedef enum slode_svi_kind { SLODE_SVI_MAIN = 0 /* SVI(model, guide) */, SLODE_SVI_AUX = 1 /* SVI(model_meta, guide_meta) */ } slode_svi_kind;
/* = slode_elbo_step / slode_elbo_adam_step (kind MAIN) or slode_aux_step (kind AUX) on a slode_batch.  grads == NULL: loss only
 * (SVI.evaluate_loss); adam != NULL: the update is applied by the final reduction kernel (grads must be given).  times / stage_t are
 * ignored for kind AUX. */
int slode_svi_step(slode_handle h, const slode_shape* s, const slode_layout* lay, int kind, float* params, const float* times,
                   const float* stage_t, const slode_batch* batch, float* loss_out, float* grads, void* workspace, size_t workspace_bytes,
                   const slode_adam* adam, void* stream);

/* ---- one batch of the per-epoch statistics as ONE call (training_cvs.py:43-144 `input_pred_stats`: evaluate_loss of both SVI objects, recon,
 * classifier / pred_inputs; four such passes per epoch, :270-315) ---------------------------------------------------------------------------
 * Writes one row of SLODE_EVAL_SLOTS floats to device memory:
 *   out[0]      -ELBO of the main loss, summed over the batch          (= slode_svi_step, kind MAIN, grads NULL)
 *   out[1]      auxiliary loss, summed over the batch; 0 with n_aux = 0 (= slode_svi_step, kind AUX, grads NULL)
 *   out[2]      sum over [B, C, T] of |centre curve - observation|: mu_50 (ALD) or mean (Gauss) of the reconstruction of ONE latent draw --
 *               is_post != 0: from the posterior N(loc(x), scale(x)); is_post == 0: from the conditional prior p(z | labels), N(0, 1) on the
 *               dims outside every prior group (= recon(is_post)["l1"] * B * C * T, models/mechanistic_cvs.py:298-323)
 *   out[3 + a]  a < n_aux: trajectories whose prediction of label head a (the order of slode_shape::aux) is a hit.  Prediction from one
 *               posterior draw, as classifier / pred_inputs decide it (mechanistic_cvs.py:278-296): SIGMOID: p > 0.5; SOFTMAX: one-hot of
 *               the arg-max, lowest index on a tie; EXPEXP: the Laplace location, the value slode_label_heads writes.  Hit: every column
 *               within 0.5 of the label.  Slots of absent heads: 0.
 *   out[7]      B
 * Four independent latent draws per trajectory, in the order main, auxiliary, recon, labels: batch->eps == NULL takes drawing calls n, n + 1,
 * n + 2, n + 3 of the handle's generator and leaves the counter at n + 4 -- what the unfused sequence of calls consumes, so from the same
 * (seed, first_trajectory, n) the row equals theirs up to fp32 summation order; batch->eps != NULL is a dense [4, B, L] tensor in that order.
 * Enqueue only (no allocation, no synchronisation, capturable); at most four launches ("weff", "enc_fwd2", "eval_stats", "eval_reduce" in
 * slode_profile_read): the encoder runs once; one partial row per workgroup, summed in a fixed order: bitwise reproducible.
 * Takes the fixed-grid methods, one particle, the two dense observation layouts of the folded encoder ([B,T,C] or [B,C,T] contiguous, C in
 * {3, 4}).  Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: adaptive solver (dopri5, bosh3,
 * fehlberg2, adaptive_heun); particles > 1; observation strides the folded path does not take (and SLODE_NO_FOLD); the measured arms
 * SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG set in the environment of slode_create.  The caller then runs the unfused calls.
 * Workspace: slode_workspace_bytes of the shape (unchanged: the partial rows live in the ELBO step's slab rows). */
int slode_eval_stats(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                     const float* stage_t, const slode_batch* batch, int is_post, float* out /* [SLODE_EVAL_SLOTS] */, void* workspace,
                     size_t workspace_bytes, void* stream);

/* ---- the Monte-Carlo summary of `multiple_samples` as ONE call (training_proc.py:205-223: num_samples = config.num_samples = 200 calls of recon,
 * saved as mu_50_post_sample.npy & co.; the evaluation notebook reduces them at once with np.mean(..., 2) / np.std(..., 2)) -----------------------
 * Per trajectory, the sample moments of every decoder head curve over num_samples latent draws: mean[q][b][c][t] and sd[q][b][c][t] (T contiguous;
 * sd may be NULL), sd the POPULATION standard deviation (divisor num_samples: np.std's default); num_samples = 1 gives sd = 0 exactly and mean =
 * that draw's curve.  Nothing sized num_samples x B x C x T is written anywhere: one workgroup walks the draws of its trajectory and keeps the
 * running moments of its Q x C x T values on chip, shifted by the first draw's value (no sum of squares of the values themselves).
 *   Head order: Q and the order of q are those of slode_layout::head_w, as in slode_decode_heads -- SLODE_ALD: Q = 3, q = 0: mu_50 (output_q50),
 *   q = 1: mu_75 (output_q75), q = 2: mu_25 (output_q25); SLODE_GAUSS: Q = 1, q = 0: mean (output_mean).
 *   is_post != 0: draws from the posterior N(loc(x), scale(x)) -- three launches ("weff", "enc_fwd2", "recon_moments" in slode_profile_read): the
 *   encoder runs once, as in slode_eval_stats.  is_post == 0: draws from the conditional prior p(z | labels), N(0, 1) on the dims outside every
 *   prior group -- ONE launch ("recon_moments"): the encoder does not run, batch->obs may be NULL and its strides are not read.
 *   Noise: batch->eps == NULL uses ONE drawing call n of the handle's generator -- draw k of trajectory b is row k * B + b (plus first_trajectory)
 *   of that call, i.e. slode_rng_normal(h, n, num_samples * B, L, ...) viewed as [num_samples, B, L] -- and leaves the counter at n + 1;
 *   batch->eps != NULL is a dense [num_samples, B, L] tensor.  The result is a function of (parameters, inputs, noise) alone: independent of the
 *   grid, bitwise reproducible from run to run (every value has one owner thread, which takes the draws in the order k = 0 .. num_samples - 1).
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: a NULL handle (before anything else);
 * num_samples < 1 (and B x num_samples beyond 2^30 - 1 noise rows); adaptive solver (dopri5, bosh3, fehlberg2, adaptive_heun); particles > 1;
 * posterior with observation strides the folded encoder path does not take ([B,T,C] or [B,C,T] contiguous, C in {3, 4}) or under SLODE_NO_FOLD;
 * the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG set in the environment of slode_create; LDS tables (step table 2 (T - 1) S,
 * moments 3 Q C T, staged weights) beyond the budget of 160 KiB.  The caller then reduces slode_ode_solve_fwd + slode_decode_heads itself. */
int slode_recon_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                        const float* stage_t, const slode_batch* batch, int is_post, int num_samples, float* mean /* [Q,B,C,T] */,
                        float* sd /* [Q,B,C,T] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-trajectory -ELBO and importance-weighted bounds from K latent draws as ONE call (no reference counterpart: the reference's losses are
 * sums over the batch; what a user asks of a test set -- which subjects the model explains badly, a held-out log-likelihood estimate, an outlier
 * score -- is per trajectory) -------------------------------------------------------------------------------------------------------------------
 * For trajectory b and draw k, z = loc(x_b) + scale(x_b) eps[k][b], loss[k][b] is the main loss of that single row:
 *   -(log-likelihood + log p(z | labels) - log q(z | x)), plus the 46 x label terms where the main model scores the labels (aux_in_main: proc)
 * -- separable over rows, so sum_b loss[k][b] = slode_svi_step(kind MAIN, grads NULL) on that noise.  Written per trajectory:
 *   bounds[b][0]  mean over k of loss[k][b]: the trajectory's -ELBO, the summand of Trace_ELBO(num_particles = K).evaluate_loss
 *   bounds[b][1]  -log(1/K sum_k exp(-loss[k][b])): the importance-weighted bound (IWAE); <= bounds[b][0], equal to it at K = 1
 *   bounds[b][2]  effective sample size (sum w)^2 / sum w^2 of w_k = exp(-loss[k][b] + min_k loss[k][b]); in [1, K], exactly 1 at K = 1
 *   bounds[b][3]  mean over k of the negative log-likelihood term alone (bounds[b][0] - bounds[b][3]: the KL-and-label part)
 * and, when loss_kb != NULL, every loss[k][b] itself ([num_draws, B]).  bounds must be 16-byte aligned (one 16-byte store per row).
 * Posterior draws only.  Noise: batch->eps == NULL uses drawing calls n .. n + K - 1 of the handle's generator -- draw k of trajectory b is row b
 * of call n + k, the convention of slode_svi_step with particles = K -- and leaves the counter at n + K; batch->eps != NULL is a dense [K, B, L]
 * tensor.  One workgroup walks the K draws of its trajectory; the K losses are kept on chip and reduced in fp64 in a fixed order: the result is a
 * function of (parameters, inputs, noise) alone -- bitwise equal from run to run, for every grid, for in-kernel and explicit noise.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Three launches ("weff", "enc_fwd2", "traj_bounds" in
 * slode_profile_read): the encoder runs once per trajectory, not once per draw.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: a NULL handle (before anything else);
 * num_draws < 1 (and B x num_draws beyond 2^30 - 1 noise rows); adaptive solver (dopri5, bosh3, fehlberg2, adaptive_heun); particles > 1 in the
 * shape (the draws are num_draws); observation strides the folded encoder path does not take ([B,T,C] or [B,C,T] contiguous, C in {3, 4}) or
 * SLODE_NO_FOLD; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG set in the environment of slode_create; LDS tables (step table
 * 2 (T - 1) S, observations and likelihood scales 3 C T, staged weights, the 2 K per-draw values) beyond the budget of 160 KiB.  There is no
 * composed fallback: no other call returns a per-trajectory loss. */
int slode_traj_bounds(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                      const float* stage_t, const slode_batch* batch, int num_draws, float* bounds /* [B, SLODE_BOUND_SLOTS] */,
                      float* loss_kb /* [num_draws, B] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- label evidence: V label hypotheses scored per trajectory as ONE call (no reference counterpart: the reference predicts labels with the
 * auxiliary heads q(label | z_g) alone; the conditional priors p(z_g | u_g) exist to ask "which input does the generative model believe produced
 * these curves?", p(u | x) ~ p(u) p(x | u)) ------------------------------------------------------------------------------------------------------
 * hyp_labels: batch->n_labels device pointers; tensor i is a dense [V, batch->label_width[i]] table shared by all trajectories, or NULL: label i
 * is not hypothesised and every hypothesis keeps the trajectory's own tensor for it (the convention of cf_labels in slode_intervene_moments).
 * Hypothesis v for trajectory b is the label row u_b with the columns of every non-NULL tensor replaced by row v of that tensor.
 * loss[v][k][b] is the main loss of the single row b on draw k with its labels replaced by hypothesis v -- exactly what slode_traj_bounds writes
 * to loss_kb[k][b] when called with those labels and the same noise; the draws are posterior draws z = loc(x_b) + scale(x_b) eps[k][b], which do
 * not depend on the hypothesis: the encoder runs once, every draw is solved and decoded once, and a hypothesis costs its log p(z | u_v) (and, where
 * the main model scores the labels, its label log-probabilities on logits that depend on z alone).  Written per (b, v), as ONE 16-byte store:
 *   evidence[b][v][0]  mean over k of loss[v][k][b]: the -ELBO under hypothesis v
 *   evidence[b][v][1]  -log(1/K sum_k exp(-loss[v][k][b])): the importance-weighted bound on -log p(x_b | u_v)
 *   evidence[b][v][2]  effective sample size of those weights, in [1, K] -- per hypothesis: q(z | x) is a poor proposal for a wrong u, and the
 *                      ESS says when the bound is one draw wide
 *   evidence[b][v][3]  log_post = log_prior[v] - slot 1 - logsumexp_v'(log_prior[v'] - slot 1 [v']); log_prior == NULL: all 0.  Formed in fp64
 *                      from the fp64 bounds before they are rounded, in the order v = 0 .. V - 1; exactly 0 at V = 1
 * best[b] (or NULL): the arg-max over v of log_post, the lowest index on a tie.  loss_vkb (or NULL): every loss[v][k][b], [V, num_draws, B].
 * Slots 0-2 of column v and loss_vkb[v] are bit for bit what slode_traj_bounds returns for that label set on the same noise (both kernels execute
 * the same routines).  Noise: as slode_traj_bounds (batch->eps == NULL: drawing calls n .. n + K - 1, the counter left at n + K; else a dense
 * [K, B, L] tensor).  The result is a function of (parameters, inputs, hypotheses, noise) alone: bitwise equal from run to run, for every grid,
 * for in-kernel and explicit noise.  No atomics.  Enqueue only: no allocation, no synchronisation, no read-back; capturable as a linear graph.
 * Three launches ("weff", "enc_fwd2", "label_evidence" in slode_profile_read).  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_traj_bounds refuses -- a
 * NULL handle (before anything else); num_draws < 1 (and B x num_draws beyond 2^30 - 1 noise rows); adaptive solver; particles > 1; the measured
 * arms; batch->obs NULL; observation strides the folded encoder path does not take or SLODE_NO_FOLD -- then: evidence NULL or not 16-byte aligned;
 * V outside [1, SLODE_EVIDENCE_MAX_V]; hyp_labels NULL, or every entry NULL; batch->n_labels == 0; LDS tables (step table, observations, staged
 * weights, the V prior rows 3 V L, the K V losses) beyond the budget of 160 KiB.  There is no composed fallback: the composed route is V
 * slode_traj_bounds calls, which refuse the same shapes. */
int slode_label_evidence(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                         const float* stage_t, const slode_batch* batch, int num_draws, const float* const* hyp_labels, int V,
                         const float* log_prior /* device [V] or NULL */, float* evidence /* [B, V, SLODE_EVIDENCE_SLOTS] */,
                         int32_t* best /* [B] or NULL */, float* loss_vkb /* [V, num_draws, B] or NULL */, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- posterior refinement: per-trajectory ELBO ascent as ONE call (no reference counterpart: the reference's posterior is the encoder's one
 * amortised pass; closing the amortisation gap for one subject, or fitting a subject whose record is only partly trusted or observed -- a prefix of
 * the window, a dropped channel -- needs an optimiser on that subject's own q(z | x)) -----------------------------------------------------------
 * Per trajectory b, with phi = (loc[L], rho[L]), scale = exp(rho), and num_draws noise rows eps[k][b] that are FIXED for the whole call:
 *   F(phi) = 1/K sum_k loss_k,  loss_k = -(sum_{c,t,q} w[b][c][t] ll[c][t][q] + log p(z_k | labels) - log q(z_k)),  z_k = loc + exp(rho) eps[k][b]
 * -- the per-draw loss of slode_traj_bounds with a weight w >= 0 on every likelihood term of (c, t).  mask: the weights, a tensor with the
 * observations' strides (batch->obs_strides), or NULL: every weight 1, bit for bit what an all-ones mask gives.  The encoder still reads the whole
 * observation block: the mask enters the objective alone.  phi_0 = the encoder's (loc, log scale); for j = 0 .. num_steps - 1: F_j and dF/dphi from
 * the K draws (forward solve, then the reverse of it: likelihood gradient on the states, reverse affine scan, reverse of the step coefficients and
 * of the a / d evaluator, the hidden layer, the init net, the KL terms), one Adam step with lr, beta = (0.9, 0.999), eps 1e-8 and bias
 * correction; one more forward pass gives F_J.  Written: the BEST iterate (arg-min over j = 0 .. num_steps of F_j, the lowest j on a tie)
 *   loc_out [B, L], scale_out [B, L]; elbo_out [B, 2] = (F_0, the best F): elbo_out[b][1] <= elbo_out[b][0] by construction; num_steps = 0
 *   returns the encoder's loc / scale bit for bit and F_0 twice
 *   grad0_out (or NULL) [B, 2 L] = dF_0 / d(loc, rho); trace_out (or NULL) [num_steps + 1, B] = every F_j; best_step (or NULL) [B] = the arg-min
 * Noise: as slode_traj_bounds (batch->eps == NULL: drawing calls n .. n + K - 1, the counter left at n + K -- NOT n + K J; else a dense [K, B, L]
 * tensor).  The whole iteration of a trajectory runs in one workgroup with weights, observations and every table on chip; every sum runs in a
 * fixed order: the result is a function of (parameters, inputs, mask, noise) alone -- bitwise equal from run to run, for every grid, for
 * in-kernel and explicit noise.  No atomics.  Enqueue only: no allocation, no synchronisation, no read-back; capturable as a linear graph.  Three
 * launches ("weff", "enc_fwd2", "posterior_refine" in slode_profile_read).  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_traj_bounds refuses -- a
 * NULL handle (before anything else); num_draws < 1 (and B x num_draws beyond 2^30 - 1 noise rows); adaptive solver; particles > 1; the measured
 * arms; batch->obs NULL; observation strides the folded encoder path does not take or SLODE_NO_FOLD -- then: num_steps < 0; lr not finite or
 * <= 0; loc_out / scale_out / elbo_out NULL; a shape whose main loss scores the labels (aux_in_main: the proc family -- the backward pass of the
 * label heads is out of scope); LDS tables (step table and its kept copy 3 (T - 1) S, lambda T S, the stage-gradient table 2 S (T - 1) x stages,
 * observations, weights and likelihood scales 4 C T, staged weights, the K per-draw losses) beyond the budget of 160 KiB.  There is no composed
 * fallback: no other call differentiates the per-trajectory loss with respect to the posterior. */
int slode_posterior_refine(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                           const float* stage_t, const slode_batch* batch, int num_draws, int num_steps, float lr,
                           const float* mask /* as batch->obs, or NULL */, float* loc_out /* [B, L] */, float* scale_out /* [B, L] */,
                           float* elbo_out /* [B, 2] */, float* grad0_out /* [B, 2 L] or NULL */, float* trace_out /* [num_steps + 1, B] or NULL */,
                           int32_t* best_step /* [B] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- pointwise predictive density: per-point lppd and the WAIC terms from K latent draws as ONE call (no reference counterpart: the other
 * eval-side calls reduce over the observation points or over the draws before anything leaves the chip; which time points and channels of a
 * subject are surprising, the log predictive density of held-out points, and a predictive comparison of two fitted models -- WAIC / elpd -- need
 * the density per point) ---------------------------------------------------------------------------------------------------------------------------
 * For trajectory b, draw k and point i = (c, t), l_k[i] is the sum over the Q heads of the log-likelihood terms of that point (ALD: its three
 * quantile heads; Gauss: its one head) on z_k = loc + scale eps[k][b].  With normalised draw weights w_k, point [3, B, C, T] holds the planes
 *   point[0] lppd[i]    = log sum_k w_k exp(l_k[i])
 *   point[1] mean_ll[i] = sum_k w_k l_k[i]
 *   point[2] var_ll[i]  = sum_k w_k (l_k[i] - mean_ll[i])^2, the point's WAIC penalty (elpd_waic = lppd - var_ll)
 * weights: SLODE_PW_POSTERIOR: w_k = 1 / K, the draws of q(z | x) as they come, one sweep, no KL term.  SLODE_PW_IMPORTANCE: w_k ~ exp(-loss_k),
 * self-normalised, loss_k the per-draw loss of slode_traj_bounds (label terms included where the main loss has them) with the mask's weights on
 * its likelihood terms: one sweep forms the K losses exactly as slode_traj_bounds does (mask NULL: loss_kb is bit for bit its loss_kb, slot 7 its
 * ESS), the log-weights are formed in fp64 in a fixed order, and a second sweep redraws the same noise and folds the points.
 * mask: a tensor with the observations' strides, or NULL (all ones; the same instructions).  It says which points count as observed: its weights
 * multiply the likelihood terms inside loss_k (importance mode only), and it partitions the sums of summary into in (w > 0) and out (w == 0).
 * The planes are written for every point, unweighted.  loc / scale ([B, L] each, both or neither): the posterior the draws come from, e.g. the
 * output of slode_posterior_refine; NULL: the encoder's.  summary [B, SLODE_POINTWISE_SLOTS], 16-byte aligned, fp64 sums of the written plane
 * values in a fixed order that depends on (C, T) alone, rounded once, as two 16-byte stores:
 *   [0] sum_in lppd   [1] sum_in var_ll (p_waic)   [2] sum_in mean_ll   [3] n_in   [4] sum_out lppd   [5] sum_out mean_ll   [6] n_out
 *   [7] effective sample size of the weights (exactly K in posterior mode)
 * At K = 1: lppd == mean_ll bit for bit, var_ll == 0, the ESS 1.  loss_kb (or NULL; importance mode only): every loss[k][b], [num_draws, B].
 * Noise: as slode_traj_bounds, in both modes (batch->eps == NULL: drawing calls n .. n + K - 1, the counter left at n + K; else a dense [K, B, L]
 * tensor).  Every output is a function of (parameters, inputs, mask, posterior, noise) alone: bitwise equal from run to run, for every grid,
 * for in-kernel and explicit noise.  No atomics.  Enqueue only: no allocation, no synchronisation, no read-back; capturable as a linear graph.
 * Three launches ("weff", "enc_fwd2", "pointwise_density" in slode_profile_read; with loc / scale given the first two still run: they leave the
 * likelihood scale table).  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_traj_bounds refuses -- a
 * NULL handle (before anything else); num_draws < 1 (and B x num_draws beyond 2^30 - 1 noise rows); adaptive solver; particles > 1; the measured
 * arms; batch->obs NULL; observation strides the folded encoder path does not take or SLODE_NO_FOLD -- then: weights outside {0, 1}; point or
 * summary NULL, summary not 16-byte aligned; exactly one of loc / scale; loss_kb in posterior mode; LDS tables (step table 2 (T - 1) S,
 * observations, mask and likelihood scales 4 C T, the point accumulators 7 C T, staged weights, in importance mode 5 K per-draw values) beyond
 * the budget of 160 KiB.  slode_pointwise_plan: that figure for a shape, host arithmetic only.  There is no composed fallback. */
#define SLODE_POINTWISE_SLOTS 8
#define SLODE_PW_POSTERIOR 0
#define SLODE_PW_IMPORTANCE 1
int slode_pointwise_plan(const slode_shape* s, int num_draws, int weights, size_t* lds_bytes);
int slode_pointwise_density(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, int num_draws, int weights,
                            const float* mask /* as batch->obs, or NULL */, const float* loc /* [B, L] or NULL */,
                            const float* scale /* [B, L] or NULL */, float* point /* [3, B, C, T]: lppd | mean_ll | var_ll */,
                            float* summary /* [B, SLODE_POINTWISE_SLOTS] */, float* loss_kb /* [num_draws, B] or NULL */, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- PSIS leave-one-out: per-point elpd_loo and the Pareto khat from K latent draws as ONE call (no reference counterpart; the remedy for the
 * points where WAIC's p_waic is large, and the per-point diagnostic of whether a model comparison can be trusted: Vehtari, Gelman & Gabry 2017) ----
 * l_k[i] is slode_pointwise_density's per-draw log-density of point i = (c, t); posterior weights only.  The importance ratio of draw k for
 * leaving out point i is 1 / p(y_i | z_k).  point [3, B, C, T] holds the planes
 *   point[0] elpd_loo[i] = log sum_k w_k exp(l_k[i]), w_k the normalised Pareto-smoothed ratios
 *   point[1] khat[i]     = the fitted shape of the generalised Pareto tail; +inf where no smoothing was possible
 *   point[2] lppd[i]     = bit for bit plane 0 of slode_pointwise_density(SLODE_PW_POSTERIOR) on the same inputs and noise
 * per point: M = min(ceil(min(0.2 K, 3 sqrt K)), K - 1) (host, fp64); sorted l_(0) <= l_(1) <= ..., a_(j) = l_(0) - l_(j), cut = max(a_(M), log
 * DBL_MIN); the tail is the ranks j < M with a_(j) > cut strictly, n of them; n < 5: no smoothing, khat = +inf.  Else x = exp(a) - exp(cut) over
 * the tail, ascending; the generalised Pareto fit of Zhang & Stephens (2009) on m = 30 + floor(sqrt n) grid points with the prior of Vehtari et
 * al. (khat = (n k + 5) / (n + 10)); the tail's log-ratios replaced in rank order by s_j = min(log(sigma expm1(-khat log1p(-p_j)) / khat +
 * exp(cut)), 0), p_j = (j - 0.5) / n; a non-finite fit leaves the tail and gives khat = +inf.  Then
 *   elpd_loo = log((K - n) e^{l_(0)} + sum_j e^{s_j + l_(j)}) - log(sum_{not tail} e^{a_k} + sum_j e^{s_j}).
 * All of this runs in fp64 on chip, from the M + 1 smallest l_k of the point, which the kernel keeps sorted (tail_out, or NULL: [M + 1, B, C, T],
 * ascending along the first axis); sum_{not tail} e^{a_k} is the kept non-tail ranks in fp64 plus an fp32 running logsumexp(-l_k) over the K - M - 1
 * draws outside the kept values (no difference of sums: at khat > 1 one ratio dominates the total).
 * tile: time points per sweep over the draws (0: the fewest sweeps whose tables fit the LDS budget of 160 KiB; slode_loo_plan reports the
 * choice, the sweeps, the depth M + 1 and the LDS bytes: host arithmetic only).  Every sweep redraws the same noise and solves the whole grid: the
 * outputs are bitwise independent of the tile, the grid and of where the noise comes from.  mask, loc / scale, batch->eps, the counter (n -> n + K,
 * once): as slode_pointwise_density in posterior mode; the mask partitions the summary and never touches the planes.  summary [B, SLODE_LOO_SLOTS],
 * 16-byte aligned, fp64 sums of the written plane values in a fixed order that depends on (C, T) alone, rounded once:
 *   [0] sum_in elpd_loo   [1] sum_in lppd   [2] n_in   [3] #in{khat > 0.7} (+inf counts)   [4] max_in khat (-inf: no point in)
 *   [5] sum_out elpd_loo  [6] sum_out lppd  [7] n_out
 * No atomics.  Enqueue only; capturable as a linear graph.  Three launches ("weff", "enc_fwd2", "pointwise_loo" in slode_profile_read).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_pointwise_density
 * refuses in posterior mode up to the observation strides; then point or summary NULL, summary not 16-byte aligned; exactly one of loc / scale;
 * tile < 0 or > T; a tile, or a num_draws, whose tables do not fit the LDS.  The model layer composes where the call refuses. */
#define SLODE_LOO_SLOTS 8
int slode_loo_plan(const slode_shape* s, int num_draws, int tile, int* tile_out, int* sweeps, int* depth, size_t* lds_bytes);
int slode_pointwise_loo(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                        const float* stage_t, const slode_batch* batch, int num_draws, const float* mask /* as batch->obs, or NULL */,
                        const float* loc /* [B, L] or NULL */, const float* scale /* [B, L] or NULL */, int tile,
                        float* point /* [3, B, C, T]: elpd_loo | khat | lppd */, float* summary /* [B, SLODE_LOO_SLOTS] */,
                        float* tail_out /* [M + 1, B, C, T] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- counterfactual curves as ONE call (no reference counterpart: the reference's recon takes the whole latent from the posterior or the whole
 * latent from the conditional prior; the structured latent exists to ask "what would THIS subject's curves have looked like under THAT input?") ----
 * For trajectory b and draw k, with ONE noise row eps[k][b][0..L) shared by both arms:
 *   factual         z_f = loc(x_b) + scale(x_b) eps: exactly the posterior draw of slode_recon_moments(is_post = 1)
 *   counterfactual  z_cf[l] = z_f[l] outside every intervened prior group; inside an intervened group g:
 *                   z_cf[l] = ploc_g(u'_b) + exp(pls_g(u'_b)) eps[l] -- the group's conditional prior nets on the counterfactual labels u'
 * Both latents go through the same fixed-grid solve and decoder heads.  Over the num_samples draws, for every head value (q, c, t):
 *   cf_mean, cf_sd    mean and POPULATION sd (divisor num_samples) of the counterfactual curve v_cf
 *   eff_mean, eff_sd  mean and POPULATION sd of the PAIRED difference v_cf - v_f (not recoverable from the moments of two separate calls)
 * each [Q, B, C, T] (T contiguous) in the head order of slode_recon_moments (ALD: mu_50, mu_75, mu_25; Gauss: mean); any of the four may be NULL
 * (both effect outputs NULL: the factual arm is not run).  num_samples = 1 gives both sds = 0 exactly.  Nothing sized num_samples x B x C x T is
 * written anywhere: one workgroup walks the draws of its trajectory through both arms and keeps two sets of shifted running moments on chip.
 *   group_mask: bit g set = prior group g of the shape (slode_shape::groups) is intervened.  group_mask == 0 is accepted: cf = the factual
 *   moments, the effect exactly 0.
 *   cf_labels: batch->n_labels device pointers, a second label set in the form of batch->labels (dense [B, batch->label_width[i]] each).  Only
 *   the columns of intervened groups are read; a tensor none of whose columns an intervened group reads may be NULL, one with such a column
 *   may not (a group over several labels -- challenge, proc -- reads all of them: pass the unchanged ones as they are in batch->labels).
 *   Noise: batch->eps == NULL uses ONE drawing call n of the handle's generator -- draw k of trajectory b is row k * B + b (plus
 *   first_trajectory) of that call -- and leaves the counter at n + 1; batch->eps != NULL is a dense [num_samples, B, L] tensor.  The result is
 *   a function of (parameters, inputs, labels, noise) alone: independent of the grid, bitwise reproducible from run to run (every value has one
 *   owner thread, which takes the draws in the order k = 0 .. num_samples - 1; no atomics).
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Three launches ("weff", "enc_fwd2", "intervene_moments" in
 * slode_profile_read) on one stream.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: every refusal of slode_recon_moments(is_post = 1)
 * -- a NULL handle (before anything else); num_samples < 1 (and B x num_samples beyond 2^30 - 1 noise rows); adaptive solver (dopri5, bosh3,
 * fehlberg2, adaptive_heun); particles > 1; observation strides the folded encoder path does not take ([B,T,C] or [B,C,T] contiguous, C in
 * {3, 4}) or SLODE_NO_FOLD; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG set in the environment of slode_create; LDS tables
 * (step table 2 (T - 1) S, moments 6 Q C T, factual values Q C T, staged weights) beyond the budget of 160 KiB -- and: group_mask bits at or beyond
 * n_groups; a non-zero group_mask with cf_labels NULL (or with a NULL tensor that an intervened group reads, or with batch->n_labels == 0). */
int slode_intervene_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, const float* const* cf_labels, unsigned int group_mask,
                            int num_samples, float* cf_mean /* [Q,B,C,T] or NULL */, float* cf_sd /* [Q,B,C,T] or NULL */,
                            float* eff_mean /* [Q,B,C,T] or NULL */, float* eff_sd /* [Q,B,C,T] or NULL */, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- latent attribution as ONE call: per-block variance shares of the curves (no reference counterpart: the reference's latent is split into
 * blocks tied to the labels -- the conditional prior groups -- and the subject's own rest, z_epsilon; the structure itself asks how much of the
 * variation of a subject's curves comes from which block, at which channel and time) ----
 * Both q(z | x) and p(z | u) are diagonal Gaussians, so the blocks are independent and the variance of a curve decomposes over them (Sobol /
 * ANOVA).  The estimator is pick-freeze: redraw one set of blocks on fresh noise, keep the others, average the squared paired difference.
 *   Blocks: bit g < n_groups of a mask is prior group g of the shape (slode_shape::groups); bit n_groups is the REST block, every latent dim
 *   that no group covers.
 *   Draws: the source is that of slode_recon_moments on the same side -- is_post: loc / scale from the encoder; else the conditional prior nets on
 *   the batch's labels and N(0, 1) on the rest.  For trajectory b and draw k there are TWO noise rows, e (base) and e' (fresh):
 *     base    z[l]   = loc[l] + scale[l] e[l]
 *     arm a   z_a[l] = loc[l] + scale[l] (l in a block of arm_masks[a] ? e'[l] : e[l])
 *   Every latent goes through the same fixed-grid solve and decoder heads.  For every head value (q, c, t):
 *   mean, sd  mean and POPULATION sd (divisor num_samples) of the base curve: the quantity of slode_recon_moments, accumulated the same way;
 *             either may be NULL
 *   msd[a]    1 / (2 num_samples) sum_k (v_a,k - v_k)^2, the Jansen estimator.  A single block g in the mask: the block's TOTAL-EFFECT variance
 *             E[Var(f | z_~g)].  Every block but g in the mask: sd^2 - msd estimates the block's FIRST-ORDER variance Var(E[f | z_g]) (estimator
 *             noise can make it negative or larger than the total effect).  Every block in the mask: an independent estimate of sd^2.
 *   mean, sd [Q, B, C, T], msd [n_arms, Q, B, C, T] (T contiguous) in the head order of slode_recon_moments (ALD: mu_50, mu_75, mu_25; Gauss:
 *   mean).  arm_masks[a] == 0 is accepted and gives exactly 0: the arm runs the base's instructions on the base's z.  Nothing sized num_samples x
 *   B x C x T is written anywhere: one workgroup walks the draws of its trajectory through the base and the arms and keeps the base moments, the
 *   base values of the current draw and one sum of squares per arm on chip.
 *   arm_masks: a HOST array [n_arms] (copied into the kernel arguments at the call; not read afterwards).
 *   Noise: batch->eps == NULL: the base rows come from drawing call n of the handle's generator (row k * B + b, plus first_trajectory: exactly
 *   slode_recon_moments' draw), the fresh rows from drawing call n + 1 at the same row; the counter is left at n + 2.  batch->eps != NULL: one dense
 *   [2, num_samples, B, L] tensor, base then fresh.  The result is a function of (parameters, inputs, labels, noise, the arm's own mask) alone:
 *   independent of the grid, of where the noise comes from and of which other arms are in the call, bitwise reproducible from run to run (every
 *   value has one owner thread, which takes the draws in the order k = 0 .. num_samples - 1; no atomics).
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Posterior: three launches ("weff", "enc_fwd2", "latent_attribution"
 * in slode_profile_read) on one stream; prior: "latent_attribution" alone.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: every refusal of slode_recon_moments on that side
 * but its LDS rung -- a NULL handle (before anything else); num_samples < 1 (and B x num_samples beyond 2^30 - 1 noise rows); adaptive solver
 * (dopri5, bosh3, fehlberg2, adaptive_heun); particles > 1; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG; for the posterior,
 * batch->obs NULL, observation strides the folded encoder path does not take or SLODE_NO_FOLD; for the prior, no label tensors -- and: n_arms
 * outside [1, SLODE_ATTRIBUTION_MAX_ARMS]; arm_masks or msd NULL; a mask with bits beyond n_groups; the rest bit set when the groups cover all L
 * dims; LDS tables (step table 2 (T - 1) S, base moments 3 Q C T, base values Q C T, arm sums n_arms Q C T, staged weights, 2 L; every piece a
 * multiple of 16 B) beyond the budget of 160 KiB, naming n_arms with the figure of slode_attribution_plan. */

/* The dynamic LDS bytes of slode_latent_attribution's kernel for (shape, n_arms): pure host arithmetic -- no handle, no HIP call, works on a machine
 * without a GPU.  SLODE_EINVAL (the reason is the global text slode_last_error(NULL)) for a bad shape, n_arms outside
 * [1, SLODE_ATTRIBUTION_MAX_ARMS] or tables beyond the budget (*lds_bytes is still written then, so a caller can split its arms over calls). */
int slode_attribution_plan(const slode_shape* s, int n_arms, size_t* lds_bytes);
int slode_latent_attribution(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                             const float* stage_t, const slode_batch* batch, int is_post, int num_samples,
                             const unsigned int* arm_masks /* HOST array [n_arms], copied into the kernel arguments */, int n_arms,
                             float* mean /* [Q,B,C,T] or NULL */, float* sd /* [Q,B,C,T] or NULL */,
                             float* msd /* [n_arms,Q,B,C,T] */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- curve summaries as ONE call: peak, time to peak, area and threshold crossing of the head curves (no reference counterpart: what users of the
 * three model families ask of a curve -- how high does it get and when, how much is there in total, does it cross a level, when first and for how
 * long -- are non-linear functionals of a draw's WHOLE curve; the peak of the mean curve is not the mean of the peaks, so none of them follows from
 * the moments of slode_recon_moments) ----
 * For trajectory b, head curve q (the order of slode_recon_moments), channel c and draw k the curve is v_k(t_i), i = 0 .. T - 1, on the grid
 * `times`, with the same bits as the values slode_recon_moments accumulates.  Trapezoid node weights, formed in fp32: w_0 = 0.5 (t_1 - t_0),
 * w_i = 0.5 (t_{i+1} - t_{i-1}), w_{T-1} = 0.5 (t_{T-1} - t_{T-2}).  With the threshold thr[c] and sense (+1: "beyond" is v > thr[c]; -1:
 * v < thr[c]) the SLODE_SUMMARY_SLOTS = 8 functionals of a draw are
 *   0 peak         max_i v_i                       1 t_peak    t_i at the smallest i attaining the maximum
 *   2 trough       min_i v_i                       3 t_trough  t_i at the smallest i attaining the minimum
 *   4 auc          sum_i w_i v_i                   5 time_beyond  sum_i w_i [v_i beyond thr_c]
 *   6 t_hit        t_i at the smallest i with v_i beyond thr_c (defined only for draws that cross)
 *   7 crossed      1 if any v_i is beyond thr_c, else 0
 *   mean, sd [Q, B, C, 8]: mean and POPULATION sd of each functional over the num_samples draws, accumulated shifted by the first draw's value as
 *   in slode_recon_moments (sd may be NULL).  Slot 6 takes its moments over the crossing draws only (shifted by the first crossing draw, divided
 *   by their count) and is NaN when no draw crosses; slot 7 therefore reads P(cross) and sqrt(p (1 - p)).  num_samples = 1: every sd that is not
 *   NaN is exactly 0 and mean is that draw's functional.
 *   p_beyond [Q, B, C, T] (T contiguous) or NULL: the share of draws with v_k(t_i) beyond thr_c -- int32 counts on chip (exact), divided once.
 *   thr: a HOST array [C] (copied into the kernel arguments at the call; not read afterwards) or NULL: slots 5 - 7 are then written as NaN and
 *   p_beyond must be NULL.
 *   The sums of slots 4 and 5 have a fixed tree: time points t = l, l + 16, ... in increasing order on lane l of a 16-lane row, then the row's
 *   lanes pairwise (xor 1, xor 2, half mirror, mirror).  Extremes and first indices are comparisons and selections: exact, the smallest index
 *   wins ties.  A curve that is constant in time has t_peak = t_trough = t_0; against a threshold equal to its value it is beyond in neither
 *   sense (the comparison is strict): time_beyond = crossed = 0, t_hit NaN, p_beyond 0.
 *   Draws, sides, noise: those of slode_recon_moments -- is_post != 0: three launches ("weff", "enc_fwd2", "curve_summary" in slode_profile_read);
 *   is_post == 0: "curve_summary" alone; batch->eps == NULL: ONE drawing call n (row k * B + b, plus first_trajectory), the counter left at n + 1;
 *   else a dense [num_samples, B, L] tensor.  The result is a function of (parameters, inputs, labels, noise, thr, sense) alone: independent of the
 *   grid and of where the noise comes from, bitwise reproducible from run to run (every output has one owner thread, which takes the draws in the
 *   order k = 0 .. num_samples - 1; no atomics); mean / sd do not depend on whether sd or p_beyond is asked for.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: every refusal of slode_recon_moments on that side
 * but its LDS rung -- a NULL handle (before anything else); num_samples < 1 (and B x num_samples beyond 2^30 - 1 noise rows); adaptive solver
 * (dopri5, bosh3, fehlberg2, adaptive_heun); particles > 1; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG; for the posterior,
 * batch->obs NULL, observation strides the folded encoder path does not take or SLODE_NO_FOLD; for the prior, no label tensors -- and, after the
 * observation rungs: mean NULL; sense not +1 / -1; a non-finite thr[c]; p_beyond without thr; LDS tables (step table 2 (T - 1) S, grid and node weights 2 T,
 * value table Q C T, counts Q C T only with p_beyond, moment triples 3 Q C 8, staged weights, 2 L; every piece a multiple of 16 B) beyond the
 * budget of 160 KiB, naming whether the figure is with or without p_beyond.  The caller then reduces slode_ode_solve_fwd + slode_decode_heads
 * itself. */

/* The dynamic LDS bytes of slode_curve_summary's kernel for a shape, with (want_p_beyond != 0) or without the counters of p_beyond: pure host
 * arithmetic -- no handle, no HIP call, works on a machine without a GPU.  SLODE_EINVAL (the reason is the global text slode_last_error(NULL)) for
 * a bad shape or tables beyond the budget (*lds_bytes is still written then, so a caller can drop p_beyond). */
int slode_curve_summary_plan(const slode_shape* s, int want_p_beyond, size_t* lds_bytes);
int slode_curve_summary(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                        const float* stage_t, const slode_batch* batch, int is_post, int num_samples,
                        const float* thr /* HOST [C] or NULL */, int sense,
                        float* mean /* [Q,B,C,8] */, float* sd /* [Q,B,C,8] or NULL */, float* p_beyond /* [Q,B,C,T] or NULL */,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- counterfactual summaries as ONE call: peak, AUC and threshold crossing of every subject's curves under V hypothesised inputs, with the
 * paired effect on each functional (no reference counterpart: "by how much does input u' lower THIS subject's peak, and does the curve still
 * cross the level?" is the product of slode_intervene_moments and slode_curve_summary -- the peak of the mean counterfactual curve is not the
 * mean of the peaks, and the sd of a paired effect on a functional cannot be formed from two separate calls) ----
 * Draws: for trajectory b and draw k, on ONE noise row (row k * B + b of one drawing call, as slode_intervene_moments), z_f = loc_q + scale_q eps.
 * Arms: for v < V, z_cf,v = z_f outside the prior groups of group_mask and ploc_g(u'_{b,v}) + exp(pls_g(u'_{b,v})) eps inside them, with the bits
 * slode_intervene_moments forms for the same labels.  Hypotheses: u'_{b,v} is row b's own label row with the columns of every non-NULL entry of
 * hyp_labels (one entry per label tensor of the batch, a dense [V, width] table shared by all trajectories) replaced by row v of that table:
 * the convention of slode_label_evidence.
 * All V + 1 latents go through the same fixed-grid solve and heads; per head curve q, channel c and arm the eight functionals of a draw are
 * exactly those of slode_curve_summary (same trapezoid node weights, same 16-lane walk and combine order -- xor 1, xor 2, half mirror, mirror
 * --, the smallest i wins ties, same thr / sense).  Call them f_f[s] and f_v[s], s = 0 .. 7.  Three sets of shifted moments over the draws
 * (mean and POPULATION sd, accumulated as in slode_recon_moments) are written:
 *   f_mean, f_sd      [Q, B, C, 8]     the factual arm: bit for bit what slode_curve_summary(is_post = 1) writes on the same noise
 *   cf_mean, cf_sd    [V, Q, B, C, 8]  arm v; slot 6 (t_hit) over that arm's crossing draws, NaN where none crosses
 *   eff_mean, eff_sd  [V, Q, B, C, 8]  the paired difference e = fl(f_v[s] - f_f[s]): slots 0 - 5 and 7 over all draws, slot 7 the difference
 *                                      of the two indicators in {-1, 0, 1}; slot 6 over the draws that cross in BOTH arms (shifted by the first
 *                                      of them, divided by their count), NaN for mean and sd where there is none
 *   Hence eff_mean[7] = P_cf - P_f (the change of P(cross)), and eff_sd[7]^2 + eff_mean[7]^2 = mean of e^2 = the share of draws whose crossing
 *   changes.  Every output but cf_mean may be NULL; with f_* and eff_* all NULL the factual arm is not run.
 *   thr: a HOST array [C] (copied into the kernel arguments at the call) or NULL: slots 5 - 7 of all three sets are then NaN.
 *   group_mask = 0 (hyp_labels is then not read): every arm runs on z_f through the same instructions, cf == f bitwise and every effect is 0.
 *   num_samples = 1: every sd that is not NaN is exactly 0.
 *   Column v is bitwise independent of V and of the other rows of the tables: arm v of a V-arm call equals the V = 1 call with that row, so
 *   more hypotheses than one call holds may be split over calls on the same noise.
 *   Noise: batch->eps == NULL: ONE drawing call n (row k * B + b, plus first_trajectory), the counter left at n + 1; else a dense
 *   [num_samples, B, L] tensor.  Three launches ("weff", "enc_fwd2", "intervene_summary" in slode_profile_read).  The result is a function of
 *   (parameters, inputs, labels, hypotheses, noise, thr, sense) alone: independent of the grid, of where the noise comes from and of which
 *   optional outputs are asked for, bitwise reproducible (every output has one owner thread, which takes the draws in the order
 *   k = 0 .. num_samples - 1; no atomics).
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: every refusal of slode_recon_moments for the
 * posterior but its LDS rung -- a NULL handle (before anything else); num_samples < 1; adaptive solver (dopri5, bosh3, fehlberg2,
 * adaptive_heun); particles > 1; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG; batch->obs NULL, observation strides the
 * folded encoder path does not take or SLODE_NO_FOLD -- and, after the observation rungs: cf_mean NULL; V outside
 * [1, SLODE_INTERVENE_SUMMARY_MAX_ARMS]; sense not +1 / -1; a non-finite thr[c]; group_mask bits at or beyond n_groups; a non-zero mask with
 * hyp_labels NULL or every entry NULL; a non-zero mask none of whose groups reads a column of a hypothesised tensor; LDS tables (step table
 * 2 (T - 1) S, staged weights, posterior 2 L, counterfactual 2 L V, grid and node weights 2 T, value table Q C T, factual functionals Q C 8,
 * moment triples 3 Q C 8 (1 + 2 V), the slot-6 counts Q C 2 V; every piece a multiple of 16 B) beyond the budget of 160 KiB, naming V and the
 * largest V that fits. */

/* The dynamic LDS bytes of slode_intervene_summary's kernel for a shape and V arms: pure host arithmetic -- no handle, no HIP call, works on a
 * machine without a GPU.  SLODE_EINVAL (the reason is the global text slode_last_error(NULL)) for a bad shape, V outside
 * [1, SLODE_INTERVENE_SUMMARY_MAX_ARMS] or tables beyond the budget (*lds_bytes is still written then; the text names the largest V that fits). */
int slode_intervene_summary_plan(const slode_shape* s, int V, size_t* lds_bytes);
int slode_intervene_summary(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch,
                            const float* const* hyp_labels /* n_labels pointers, each [V, width] or NULL (NULL altogether with group_mask == 0) */, int V,
                            unsigned int group_mask, int num_samples, const float* thr /* HOST [C] or NULL */, int sense,
                            float* f_mean /* [Q,B,C,8] or NULL */, float* f_sd /* [Q,B,C,8] or NULL */, float* cf_mean /* [V,Q,B,C,8] */,
                            float* cf_sd /* [V,Q,B,C,8] or NULL */, float* eff_mean /* [V,Q,B,C,8] or NULL */, float* eff_sd /* [V,Q,B,C,8] or NULL */,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- sample quantiles of the head curves as ONE call: the credible band, the envelope, the median over the draws (no reference counterpart: the
 * reference saves the [B, C, T, num_samples] curves of multiple_samples and its users take np.percentile(samples, [2.5, 97.5], axis=-1) of them;
 * mean +- 2 sd of slode_recon_moments is no substitute for the skewed prior-side curves) ----
 * For trajectory b, head curve q (the order of slode_recon_moments), channel c and time point t let v_(0) <= ... <= v_(K-1) be the K = num_samples
 * draw values, sorted -- the same bits as the values slode_recon_moments accumulates.  For a level p in [0, 1] (numpy's default "linear" definition;
 * the ranks are formed on the host in fp64):
 *   h = p (K - 1),  lo = floor(h),  hi = min(lo + 1, K - 1),  g = (float)(h - lo),
 *   out[level, q, b, c, t] = fma(g, v_(hi) - v_(lo), v_(lo))     (fp32; the difference rounded on its own, then one fma)
 * so a level with g == 0 (p = 0: the minimum, p = 1: the maximum, K = 1, p (K - 1) an integer) is one of the draw values exactly.  out is
 * [n_levels, Q, B, C, T], T contiguous; n_levels <= SLODE_QUANTILE_MAX_LEVELS = 8; levels: a HOST array [n_levels] of doubles (read at the call;
 * any order, duplicates allowed).
 *   Depths: every needed rank r (lo of every level; hi where g != 0: an upper rank without weight is not read) is served from one of two sorted buffers per value, kept in the LDS: the depth_lo smallest draws so far (cost
 *   r + 1) or the depth_hi largest (cost K - r), whichever costs less, the bottom one on a tie; depth_lo / depth_hi: the largest cost given to a
 *   side; depth_lo + depth_hi >= K: every draw is kept (depth_lo = K, depth_hi = 0).  (0.025, 0.975) at K = 200: 6 + 6; (0, 1): 1 + 1; a median
 *   at K = 200: 200.
 *   Tiles: the buffers [depth][Q C][tile] hold `tile` time points; T > tile takes sweeps = ceil(T / tile) passes over the draws, each solving
 *   the whole grid on the same noise.  tile = 0: the fewest sweeps that fit the LDS budget of 160 KiB, tile = ceil(T / sweeps); tile > 0: as given.
 *   Draws, sides: those of slode_recon_moments -- is_post != 0: three launches ("weff", "enc_fwd2", "recon_quantiles" in slode_profile_read);
 *   is_post == 0: "recon_quantiles" alone.  Noise: batch->eps == NULL: row k * B + b (plus first_trajectory) of drawing call n, as
 *   slode_recon_moments; the counter is left at n + num_samples, whatever the number of sweeps; else a dense [num_samples, B, L] tensor.
 *   The result is a function of (parameters, inputs, labels, noise, levels) alone: bitwise independent of the grid, of the tile and of where the
 *   noise comes from (every output has one owner thread, which takes the draws in the order k = 0 .. num_samples - 1; no atomics).  Non-finite
 *   curve values are not ordered: the outputs of such a (q, b, c, t) are unspecified.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: every refusal of slode_recon_moments on that side
 * but its LDS rung -- a NULL handle (before anything else); num_samples < 1 (and B x num_samples beyond 2^30 - 1 noise rows); adaptive solver
 * (dopri5, bosh3, fehlberg2, adaptive_heun); particles > 1; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG; for the posterior,
 * batch->obs NULL, observation strides the folded encoder path does not take or SLODE_NO_FOLD; for the prior, no label tensors -- and, after the
 * observation rungs: out NULL; n_levels outside [1, 8]; levels NULL; a level outside [0, 1] or NaN; tile < 0 or tile > T; a given tile whose
 * tables (step table 2 (T - 1) S, staged weights, 2 L, level table, buffers depth Q C tile; every piece a multiple of 16 B) exceed the budget;
 * tile = 0 where not even one time point fits.  The caller then sorts slode_ode_solve_fwd + slode_decode_heads itself. */

/* The plan of slode_recon_quantiles for (shape, num_samples, levels, tile): the tile it would use, the sweeps over the draws, the two depths and
 * the kernel's dynamic LDS bytes: pure host arithmetic -- no handle, no HIP call, works on a machine without a GPU.  SLODE_EINVAL (the reason is
 * the global text slode_last_error(NULL)) for a bad shape, a NULL output and everything the call refuses at its own rungs. */
int slode_quantile_plan(const slode_shape* s, int num_samples, int n_levels, const double* levels /* HOST [n_levels] */, int tile, int* tile_out,
                        int* sweeps, int* depth_lo, int* depth_hi, size_t* lds_bytes);
int slode_recon_quantiles(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                          const float* stage_t, const slode_batch* batch, int is_post, int num_samples, int n_levels,
                          const double* levels /* HOST [n_levels] */, int tile, float* out /* [n_levels,Q,B,C,T] */, void* workspace,
                          size_t workspace_bytes, void* stream);

/* ---- mechanism curves as ONE call: the moments of what the dynamics say at every grid point (no reference counterpart: the reference's
 * dynamics are dx/dt = a(t, z) - d(t, z) x, production a and degradation d both sigmoid outputs of one hidden layer on (t, z) -- a / d is the
 * moving set point a state relaxes towards, 1 / d its local time constant, a - d x the net rate -- yet only a - d x of one t per launch is
 * exposed, slode_dynamics_eval) ----
 * For trajectory b and draw k let x_i be the scheme's state at grid point i = 0 .. T - 1 (x_0 from the init net; the rest with the same bits as
 * the states slode_recon_moments forms its head values from) and a, d the dynamics net at times[i]: each step's first stage time stage_t[i R]
 * is bitwise times[i], stage_t[R (T - 1)] is bitwise times[T - 1].  The SLODE_MECHANISM_SLOTS = 5 slots of a draw, per state component s and
 * grid point i, in fp32:
 *   0 state        x_i[s]
 *   1 production   a_s(times[i], z)
 *   2 degradation  d_s(times[i], z)
 *   3 set_point    a / d (one correctly rounded division)
 *   4 net_rate     fmaf(-d, x_i[s], a): the vector field at the grid point
 *   slots: a bit mask over the five; n_sel: its population count.  mean, sd [n_sel, B, S, T] (T contiguous; the selected slots in increasing
 *   slot order): mean and POPULATION sd of each value over the num_samples draws, accumulated shifted by the first draw's value as in
 *   slode_recon_moments (sd may be NULL).  num_samples = 1: sd is exactly 0 and mean is the draw's value.  Non-finite values are not
 *   special-cased.
 *   Draws, sides, noise: those of slode_recon_moments -- is_post != 0: three launches ("weff", "enc_fwd2", "mechanism_moments" in
 *   slode_profile_read); is_post == 0: "mechanism_moments" alone; batch->eps == NULL: ONE drawing call n (row k * B + b, plus first_trajectory),
 *   the counter left at n + 1; else a dense [num_samples, B, L] tensor.  The result is a function of (parameters, inputs, labels, noise) alone:
 *   independent of the grid, of where the noise comes from and of which other slots are selected, bitwise reproducible from run to run (every
 *   output has one owner thread, which takes the draws in the order k = 0 .. num_samples - 1; no atomics); mean does not depend on whether sd is
 *   asked for.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: every refusal of slode_recon_moments on that side
 * but its LDS rung -- a NULL handle (before anything else); num_samples < 1 (and B x num_samples beyond 2^30 - 1 noise rows); adaptive solver
 * (dopri5, bosh3, fehlberg2, adaptive_heun); particles > 1; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG; for the posterior,
 * batch->obs NULL, observation strides the folded encoder path does not take or SLODE_NO_FOLD; for the prior, no label tensors -- and, after the
 * observation rungs: mean NULL; slots == 0 or bits at or beyond SLODE_MECHANISM_SLOTS; LDS tables (step table 2 (T - 1) S, moment triples
 * 3 S T per slot, capture table 2 T S, staged weights, 2 L; every piece and every slot's triples a multiple of 16 B) beyond the budget of 160 KiB, naming the slot count.
 * The caller then selects fewer slots per call (the same noise gives the same bits) or composes slode_ode_solve_fwd and the dynamics net. */

/* The dynamic LDS bytes of slode_mechanism_moments' kernel for a shape and a slot mask: pure host arithmetic -- no handle, no HIP call, works on
 * a machine without a GPU.  SLODE_EINVAL (the reason is the global text slode_last_error(NULL)) for a bad shape, a bad mask or tables beyond the
 * budget (*lds_bytes is still written then, so a caller can drop slots). */
int slode_mechanism_plan(const slode_shape* s, unsigned int slots, size_t* lds_bytes);
int slode_mechanism_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                            const float* stage_t, const slode_batch* batch, int is_post, int num_samples, unsigned int slots,
                            float* mean /* [n_sel,B,S,T] */, float* sd /* [n_sel,B,S,T] or NULL */,
                            void* workspace, size_t workspace_bytes, void* stream);

/* ---- simultaneous (sup-t) credible bands as ONE call (no reference counterpart: a band drawn from per-point intervals -- mean +- z sd of
 * slode_recon_moments, the quantiles of slode_recon_quantiles -- is read as "the curve lies in here with 95 % probability" and makes no such
 * claim; how much less it holds depends on how correlated the curve is along time) ----
 * For trajectory b, head curve q (the order of slode_recon_moments) and channel c let v_k(t) be the K = num_samples draw curves, m(t) and s(t)
 * their mean and population sd -- the bits slode_recon_moments returns for the same noise, written to mean / sd [Q,B,C,T] -- and
 *   dev_k = max over the participating t of  fl(fl(|v_k(t) - m(t)|) / s(t))      (fp32; a point takes part when s(t) > sd_floor; no point: 0)
 * the largest standardised deviation of draw k.  A curve whose draws coincide at every t (s = 0 everywhere) has no participating point at
 * sd_floor = 0: dev_k = 0 for every k, crit = 0, joint = 1 at every level, obs_dev = (0, 0) whatever the observations.
 * dev_k <= sqrt(K - 1) whatever the model: below about K = 20 a 95 % value is a property of K.
 * Per level p_j (levels: a HOST array [n_levels] of doubles in (0, 1], read at the call; any order, duplicates allowed; n_levels <=
 * SLODE_JOINT_BAND_MAX_LEVELS = 8), formed on the host in fp64 (slode_joint_band_levels):
 *   r_j = min(K, max(1, ceil(p_j K - 1e-9))),   z_j = Phi^-1((1 + p_j) / 2)  (p_j = 1: +inf)
 *   crit [Q,B,C,n_levels]:  the r_j-th smallest of dev_0 .. dev_{K-1}, counted from 1 -- one of the deviations exactly; mean +- crit sd holds
 *                           r_j of the K draws over the whole grid
 *   joint [Q,B,C,n_levels] (or NULL):  #{k : dev_k <= (float)z_j} / K, the share of draws wholly inside the POINTWISE band mean +- z_j sd
 *   obs_dev [Q,B,C,2] (or NULL):  [0] the deviation of the observed curve y(b, c, .) by the same formula (NaN without observations: the prior
 *                           with batch->obs == NULL), [1] the number of participating time points, an int32 stored as float
 *   dev_out [Q,B,C,num_samples] (or NULL):  dev_k itself
 *   Two sweeps over the draws, the second on the same noise (the counter-based generator redraws it; eps is read twice); each solves the whole
 *   grid.  Draws, sides: those of slode_recon_moments -- is_post != 0: three launches ("weff", "enc_fwd2", "joint_band" in slode_profile_read);
 *   is_post == 0: "joint_band" alone.  Noise: batch->eps == NULL: ONE drawing call n (row k * B + b, plus first_trajectory), the counter left
 *   where one slode_recon_moments call leaves it, whatever the sweeps; else a dense [num_samples, B, L] tensor.
 *   The result is a function of (parameters, inputs, labels, noise, levels, sd_floor) alone: bitwise independent of the grid and of where the
 *   noise comes from (every output has one owner thread; maxima and order statistics are selections; no atomics).  Non-finite curve values are
 *   not ordered: the outputs of such a curve are unspecified.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched or drawn: a NULL handle (before anything else);
 * num_samples < 2 (the sd of one draw is 0); every further refusal of slode_recon_moments on that side but its LDS rung -- B x num_samples
 * beyond 2^30 - 1 noise rows; adaptive solver; particles > 1; the measured arms SLODE_FOLD_NEXT / SLODE_ODE_PACK / SLODE_ODE_ALG; for the
 * posterior, batch->obs NULL, observation strides the folded encoder path does not take or SLODE_NO_FOLD; for the prior, no label tensors, and
 * observations (optional there) that are not dense [B,T,C] or [B,C,T] -- and, after the observation rungs: mean / sd / crit NULL; n_levels
 * outside [1, 8]; levels NULL; a level outside (0, 1] or NaN; sd_floor < 0 or not finite; LDS tables (step table 2 (T - 1) S, staged weights,
 * the table 3 Q C T, the deviations Q C num_samples, 2 L; every piece a multiple of 16 B) beyond 160 KiB.  The caller then reduces
 * slode_ode_solve_fwd + slode_decode_heads itself. */

/* The kernel's dynamic LDS bytes for (shape, num_samples): pure host arithmetic -- no handle, no HIP call, works on a machine without a GPU.
 * SLODE_EINVAL (the reason is the global text slode_last_error(NULL)) for a bad shape, num_samples < 2 or tables beyond the budget
 * (*lds_bytes is still written then). */
int slode_joint_band_plan(const slode_shape* s, int num_samples, size_t* lds_bytes);
/* The ranks r_j (counted from 1) and half-widths z_j of slode_joint_band for num_samples draws, as the call forms them: host arithmetic.
 * SLODE_EINVAL for num_samples < 2, n_levels outside [1, 8], a NULL pointer or a level outside (0, 1]. */
int slode_joint_band_levels(int num_samples, int n_levels, const double* levels /* HOST [n_levels] */, int* ranks /* [n_levels] */,
                            double* z /* [n_levels] */);
int slode_joint_band(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                     const float* stage_t, const slode_batch* batch, int is_post, int num_samples, int n_levels,
                     const double* levels /* HOST [n_levels] */, float sd_floor, float* mean /* [Q,B,C,T] */, float* sd /* [Q,B,C,T] */,
                     float* crit /* [Q,B,C,n_levels] */, float* joint /* [Q,B,C,n_levels] or NULL */, float* obs_dev /* [Q,B,C,2] or NULL */,
                     float* dev_out /* [Q,B,C,num_samples] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- forecast: the posterior (or prior) curves of a trained model on ANY output grid as ONE call (no reference counterpart: the reference solves
 * on the training grid alone; what one asks of a latent ODE first is what this subject's curves look like after the observed window, or on a
 * finer grid) ------------------------------------------------------------------------------------------------------------------------------------
 * slode_shape::T stays what the model was trained with -- the encoder's input length, the row length of constant_std, the parameter layout --
 * and the output grid is an argument of its own. */

/* slode_stage_times for a grid of n_times points that need not equal s->T: the same kernel and the same fp32 arithmetic, run on a shape copy
 * with T = n_times.  Of `s` only the method matters.  2 <= n_times <= SLODE_FORECAST_MAX_T.  times[n_times] ->
 * stage_t[slode_num_stage_times_n(s, n_times)] (R * (n_times - 1) + 1; SLODE_EINVAL, negative, for n_times out of range). */
int slode_num_stage_times_n(const slode_shape* s, int n_times);
int slode_stage_times_n(slode_handle h, const slode_shape* s, int n_times, const float* times, float* stage_t, void* stream);

/* The window slode_forecast_moments will use for (shape, T_out, num_samples, want_states, window) and the dynamic LDS bytes of its kernel: pure
 * host arithmetic -- no handle, no HIP call, works on a machine without a GPU.  The kernel walks the output grid in windows of *window_out grid
 * steps; the LDS holds, beside the staged weights, loc | scale and the carry table [num_samples][S], one window's tables only: step table
 * 2 W S, moments 3 Q C (W + 1), state moments 3 S (W + 1) when want_states (every piece a multiple of 16 B; budget 160 KiB).
 *   window > 0: clamped to T_out - 1 and used as given; SLODE_EINVAL naming the window if its tables do not fit.
 *   window == 0: the whole grid (T_out - 1 steps) if it fits; else the largest multiple of 256 steps that fits; failing that the largest
 *   multiple of 64; failing that the largest that fits; SLODE_EINVAL naming num_samples if not one step fits beside the carry table.
 * On refusal the reason is the global text slode_last_error(NULL).  (A handle created under SLODE_ODE_GENERIC sizes the staged rows for the
 * largest S: the call's own plan can then come out smaller than this one.) */
int slode_forecast_plan(const slode_shape* s, int T_out, int num_samples, int want_states, int window, int* window_out, size_t* lds_bytes);

/* Per trajectory, the sample moments over num_samples latent draws of every decoder head curve -- and of the ODE state -- on the output grid
 * times_out[0 .. T_out): mean[q][b][c][t] and sd[q][b][c][t] (T_out contiguous; POPULATION sd; head order of slode_recon_moments; sd may be
 * NULL) and x_mean[b][s][t], x_sd[b][s][t], the same moments of the state x (recon's solution_xt; either or both may be NULL, both NULL: the
 * state tables are not kept).
 *   The draws are those of slode_recon_moments: is_post != 0 from the posterior N(loc(x), scale(x)) of the observations on the shape's own T
 *   (launches "weff", "enc_fwd2", "forecast_moments" in slode_profile_read); is_post == 0 from the conditional prior p(z | labels) (ONE launch,
 *   "forecast_moments"; batch->obs may be NULL).  times / stage_t are the training grid's tables, as every eval-side call takes them.
 *   The solve and the heads run on times_out with the shape's fixed-grid method, stage_t_out from slode_stage_times_n(h, s, T_out, times_out, ..).
 *   The initial state x0 = initialize_state(z) is the state AT times_out[0], as odeint(f, x0, times) places it: a forecast grid begins at the
 *   training grid's first time.  times_out must be strictly monotone; as with `times`, a table that is not gives NaN.  T_out is independent of
 *   s->T in both directions, 2 <= T_out <= SLODE_FORECAST_MAX_T (beyond the 1024 of slode_shape::T too).  No observation noise is added:
 *   constant_std exists on the training grid only.
 *   window: grid steps solved per pass, 0 = the library's choice (slode_forecast_plan, with x_mean / x_sd deciding want_states).  The grid is
 *   walked windows outer, draws inner: every draw's latent is formed again per window from the same noise, and only its state at the window's
 *   last point is carried.  The result does not depend on the launch grid and is bitwise reproducible for a given window; two windows agree to
 *   fp32 rounding (the window decides how the scan associates the steps' affine maps).  With times_out = times and one window the operations
 *   are those of slode_recon_moments.
 *   Noise: exactly slode_recon_moments' -- batch->eps == NULL: ONE drawing call n, draw k of trajectory b is row k * B + b, counter left at
 *   n + 1; batch->eps != NULL: a dense [num_samples, B, L] tensor.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_recon_moments refuses
 * for the same is_post except its LDS rung (a NULL handle first; num_samples < 1; B x num_samples beyond 2^30 - 1; adaptive solver;
 * particles > 1; the measured arms; posterior strides / SLODE_NO_FOLD); then times_out / stage_t_out NULL; T_out outside
 * [2, SLODE_FORECAST_MAX_T]; mean NULL; window < 0; the plan's refusal.  The caller then reduces slode_ode_solve_fwd on a shape with T = T_out
 * (it reads no T-sized parameter) and the head products itself. */
int slode_forecast_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                           const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const float* times_out,
                           const float* stage_t_out, int T_out, int window, float* mean /* [Q,B,C,T_out] */,
                           float* sd /* [Q,B,C,T_out] or NULL */, float* x_mean /* [B,S,T_out] or NULL */, float* x_sd /* [B,S,T_out] or NULL */,
                           void* workspace, size_t workspace_bytes, void* stream);

/* ---- forecast summaries: "will the curve cross the level AFTER the observed window, when, how high will it still get and how much is still
 * to come?"  The moments of slode_forecast_moments do not answer it -- the peak of the mean forecast is not the mean of the peaks, P(cross) is
 * no function of mean +- sd -- and forecast_samples reduced by the caller materialises [B, C, T_out, K] and stops at T_out = 1024. */

/* The window slode_forecast_summary will use for (shape, T_out, window) and the dynamic LDS bytes of its kernel: pure host arithmetic, as
 * slode_forecast_plan.  The LDS holds the staged weights, loc | scale, ONE carry [S], one window's tables -- step table 2 W S, grid and node
 * weights 2 (W + 1), values Q C (W + 1) -- and the moment triples 3 Q C 8 (every piece a multiple of 16 B; budget 160 KiB).  There is no
 * num_samples term: the kernel walks a draw through all its windows before the next draw starts.  The ladder is slode_forecast_plan's:
 *   window > 0: clamped to T_out - 1 and used as given; SLODE_EINVAL naming the window if its tables do not fit.
 *   window == 0: the whole grid if it fits; else the largest multiple of 256 steps that fits; failing that the largest multiple of 64;
 *   failing that the largest that fits. */
int slode_forecast_summary_plan(const slode_shape* s, int T_out, int window, int* window_out, size_t* lds_bytes);

/* Per trajectory b, head curve q and channel c: the mean and the POPULATION sd over num_samples latent draws of the SLODE_SUMMARY_SLOTS = 8
 * functionals of slode_curve_summary (same slot order and meaning), taken on the sub-grid times_out[first_point .. T_out) of the draw's curve
 * v_k(t) as slode_forecast_moments solves it (the shape's fixed-grid method, x0 at times_out[0], stage_t_out from slode_stage_times_n):
 *   peak, trough        the extreme over the points g >= first_point; t_peak, t_trough: the grid time of the FIRST point attaining it
 *   auc                 the trapezoid rule on the sub-grid: sum of w[g] v[g], w[g] = 0.5f * (t[min(g + 1, T_out - 1)] - t[max(g - 1, first_point)])
 *                       (a one-point sub-grid gives 0)
 *   time_beyond         sum of w[g] over the points beyond thr[c] (sense +1: v > thr, -1: v < thr)
 *   t_hit               the time of the first point g >= first_point beyond the threshold -- a draw already beyond at first_point hits there --
 *                       mean / sd over the crossing draws only, NaN where none crosses
 *   crossed             the share of draws that cross: P(cross)
 *   mean, sd [Q, B, C, 8]; sd may be NULL; slots 5-7 are NaN with thr == NULL (thr: HOST [C] finite values, read before the call returns).
 *   There is no p_beyond[T_out] output: it would need a T_out-sized table per trajectory, and slode_forecast_moments on indicator curves is
 *   not this call's business.
 *   The draws, the noise and the counter advance (ONE drawing call) are those of slode_recon_moments / slode_forecast_moments for the same is_post;
 *   launches "weff", "enc_fwd2", "forecast_summary" (posterior) or "forecast_summary" alone (prior).
 *   window: as slode_forecast_moments (0: slode_forecast_summary_plan's choice).  The kernel walks draws outer, windows inner and merges the
 *   windows' functionals in time order (an extreme moves on strict improvement and carries its time; auc / time_beyond add in window order;
 *   the first hit stays).  Bitwise reproducible for a given window and independent of the launch grid; two windows agree to fp32 rounding.
 *   With one window, first_point = 0 and times_out = times the result is bit for bit slode_curve_summary's.  Neither num_samples nor T_out
 *   sizes anything in the LDS.
 * Enqueue only: no allocation, no synchronisation, no read-back; capturable.  Workspace: slode_workspace_bytes of the shape (unchanged).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written, in this order: everything
 * slode_forecast_moments refuses for the same is_post up to its grid (times_out / stage_t_out NULL; T_out outside [2, SLODE_FORECAST_MAX_T]);
 * first_point outside [0, T_out - 1]; sense not +-1 (then a thr that is not finite); mean NULL; window < 0; the plan's refusal. */
int slode_forecast_summary(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                           const float* stage_t, const slode_batch* batch, int is_post, int num_samples, const float* times_out,
                           const float* stage_t_out, int T_out, int first_point, int window, const float* thr /* HOST [C] or NULL */, int sense,
                           float* mean /* [Q,B,C,8] */, float* sd /* [Q,B,C,8] or NULL */, void* workspace, size_t workspace_bytes, void* stream);

/* ---- cohort curves: per-condition moments and the evaluation notebooks' L1 as ONE call (cvs_eval_final, sbio_eval_*, challenge_eval_*: the
 * subjects of one condition selected, every head curve averaged over them (and over the sample axis), np.std over the subjects for the band,
 * the observations averaged the same way, l1_error = sum_t |mean_y - mean_mu_50|) ------------------------------------------------------------
 * A cohort is a set of trajectories of the batch.  For cohort g with members b_1 .. b_n and K = num_samples draws per member, every head
 * value (q, c, t) takes v[b][k], the head curve of draw k of trajectory b: EXACTLY the draws of slode_recon_moments for the same is_post
 * (row k * B + b of one drawing call, b the trajectory's index in the batch).  With clip_min > -INFINITY, v is replaced by clip_min where
 * v < clip_min (a comparison: NaN stays NaN; the sbio notebooks' mu_50[mu_50 < 0] = 0 on the samples).
 *   mean[q][g][c][t]         mean over the n K values
 *   sd[q][g][c][t]           population sd over the n K values (divisor n K)
 *   sd_subjects[q][g][c][t]  population sd over the members of the per-member draw mean (divisor n); at K = 1 the notebooks' np.std(data[loc], 0)
 *   obs_mean[g][c][t]        mean over the members of the observation
 *   l1[g][c]                 sum_t |obs_mean[g][c][t] - mean[0][g][c][t]| (head 0 = mu_50 / the Gauss mean), in fp64 from the fp32 outputs
 * An empty cohort gives NaN in every output.  A trajectory may belong to no cohort; it must not belong to two (precondition, not checked).
 *
 * slode_cohort_plan: pure host arithmetic -- no handle, no HIP call.  chunk = R is the number of consecutive members of one cohort that one
 * workgroup folds on chip before it writes a partial: chunk in [1, SLODE_COHORT_MAX_CHUNK] is used as given; chunk == 0 lets the library
 * choose, as a function of M alone: the smallest power of two <= 64 with ceil(M / R) <= 1024.  *n_partials = ceil(M / R) + G is the bound the
 * scratch is sized by; *lds_bytes the dynamic LDS of the main kernel (budget 160 KiB: SLODE_EINVAL naming T beyond it); *scratch_bytes what
 * slode_cohort_moments needs at `scratch`.  num_samples does not enter any figure; it is checked (>= 1) only. */
int slode_cohort_plan(const slode_shape* s, int M, int G, int num_samples, int chunk, int* chunk_out, int* n_partials, size_t* lds_bytes,
                      size_t* scratch_bytes);

/* members [M] (device): the member trajectories sorted by cohort; offsets [G + 1] (device): offsets[g] .. offsets[g + 1] is cohort g's slice of
 * members, offsets[0] = 0, offsets[G] = M; 0 <= M <= B, 1 <= G <= SLODE_COHORT_MAX_G.  The host cannot check their contents; the kernels read
 * nothing out of bounds whatever they hold: offsets are clamped to [0, M] (a decreasing pair is an empty cohort), member positions to [0, M),
 * and a member index outside [0, B) is never used as an address -- it turns every output of its cohort into NaN.
 * Launches (slode_profile_read): posterior "weff", "enc_fwd2", then "cohort_plan", "cohort_moments", "cohort_merge"; the prior the last three.
 * The result is a function of (parameters, inputs, noise, members, offsets, chunk) alone: bitwise equal across runs, launch grids and in-kernel
 * vs explicit noise; two chunk sizes agree to rounding.  Noise: as slode_recon_moments (batch->eps == NULL: ONE drawing call, counter n -> n + 1;
 * else a dense [num_samples, B, L] tensor, counter unchanged).  Enqueue only, capturable, a linear graph.  scratch: 16-byte aligned device
 * memory of the plan's scratch_bytes; its contents after the call are the partials (unspecified layout).
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_recon_moments refuses
 * for the same is_post (its LDS rung replaced by this call's own); then members / offsets NULL with M > 0; M outside [0, B]; G outside
 * [1, SLODE_COHORT_MAX_G]; chunk outside [0, SLODE_COHORT_MAX_CHUNK]; mean NULL; obs_mean or l1 given with batch->obs NULL; observation
 * strides other than dense [B,T,C] / [B,C,T] whenever observations are read (the prior included); scratch NULL or misaligned; the LDS tables
 * beyond 160 KiB; and with SLODE_ENOSPC scratch_bytes below the plan's figure. */
int slode_cohort_moments(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                         const float* stage_t, const slode_batch* batch, int is_post, int num_samples,
                         const int32_t* members /* device [M] */, const int32_t* offsets /* device [G + 1] */, int M, int G, int chunk,
                         float clip_min /* -INFINITY: off */, float* mean /* [Q,G,C,T] */, float* sd /* [Q,G,C,T] or NULL */,
                         float* sd_subjects /* [Q,G,C,T] or NULL */, float* obs_mean /* [G,C,T] or NULL */, float* l1 /* [G,C] or NULL */,
                         void* scratch, size_t scratch_bytes, void* workspace, size_t workspace_bytes, void* stream);

/* ---- calibration: quantile coverage, pinball loss and band width by cohort as ONE call ------------------------------------------------------
 * The ALD families train every head curve as a quantile (P(actual < pred) = tau); the Gauss families' recon reports mean +- 2 std under the
 * same names.  Every family therefore has three curves v_0, v_1, v_2 per draw, channel and time point with nominal levels tau_0, tau_1, tau_2:
 *   ALD    the heads mu_50, mu_75, mu_25 in head order; tau = 0.5, 0.5 + quantile_diff, 0.5 - quantile_diff
 *   Gauss  mean, mean + 2 s, mean - 2 s with s = softplus(constant_std[c][t]), the scale of the likelihood; tau = 0.5, Phi(2), Phi(-2)
 *          (SLODE_CALIBRATION_PHI2 / _PHIM2)
 * The draws are EXACTLY those of slode_recon_moments / slode_cohort_moments for the same is_post; the cohorts (members, offsets, chunk) those
 * of slode_cohort_moments.  For cohort g with n members and K = num_samples draws, y the member's observation at (c, t):
 *   below[j][g][c][t]   int32: the (member, draw) pairs with y < v_j (strict: the complement of the reference's target.ge(pred))
 *   inside[g][c][t]     int32: pairs with v_2 <= y < v_1
 *   cross[g][c][t]      int32: pairs with v_2 > v_0 or v_0 > v_1 (quantile crossing; 0 by construction for the Gauss families)
 *   pinball[j][g][c]    mean over members x draws x time of (y - v_j)(tau_j - [y < v_j])
 *   width[g][c]         mean over members x draws x time of v_1 - v_2
 * An observation EQUAL to a curve value (either sign of zero against a curve that is exactly 0.0 included) is not below it: it counts in no
 * below[j], is inside only through v_2 <= y, and its pinball summand is 0; curves that are equal do not cross.
 * An empty cohort, or one with a member index outside [0, B): counts 0, float outputs NaN.  A NaN curve value compares false everywhere and
 * makes the float outputs of its cohort NaN; nothing else is affected.  M K <= B K <= 2^30 - 1 (refused beyond): int32 holds every count.
 * The integer outputs are a function of (parameters, inputs, noise, members, offsets) alone: bitwise equal across runs, launch grids, in-kernel
 * vs explicit noise AND chunk sizes.  The float outputs (fp32 summands added in fp64 in a fixed order) are bitwise equal across runs, grids
 * and the noise source; two chunk sizes agree to rounding.
 *
 * slode_calibration_plan: pure host arithmetic, the chunk rule of slode_cohort_plan (chunk == 0: a function of M alone); *n_partials =
 * ceil(M / R) + G; *lds_bytes the dynamic LDS of the main kernel (budget 160 KiB); *scratch_bytes what slode_calibration needs at `scratch`. */
int slode_calibration_plan(const slode_shape* s, int M, int G, int num_samples, int chunk, int* chunk_out, int* n_partials, size_t* lds_bytes,
                           size_t* scratch_bytes);

/* members / offsets / M / G / chunk / scratch: as slode_cohort_moments.  Launches (slode_profile_read): posterior "weff", "enc_fwd2", then
 * "cohort_plan", "calibration", "calibration_merge"; the prior the last three.  Noise: as slode_recon_moments (batch->eps == NULL: ONE drawing
 * call, counter n -> n + 1).  Enqueue only, capturable, a linear graph, no atomics.
 * Refused with SLODE_EINVAL, by name in slode_last_error, before anything is launched, drawn or written: everything slode_recon_moments refuses
 * for the same is_post (its LDS rung replaced by this call's own), with batch->obs NULL refused for BOTH is_post values; then members /
 * offsets NULL with M > 0; M outside [0, B]; G outside [1, SLODE_COHORT_MAX_G]; chunk outside [0, SLODE_COHORT_MAX_CHUNK]; below NULL;
 * observation strides other than dense [B,T,C] / [B,C,T] (the prior included); scratch NULL or misaligned; the LDS tables beyond 160 KiB; and
 * with SLODE_ENOSPC scratch_bytes below the plan's figure. */
int slode_calibration(slode_handle h, const slode_shape* s, const slode_layout* lay, const float* params, const float* times,
                      const float* stage_t, const slode_batch* batch, int is_post, int num_samples,
                      const int32_t* members /* device [M] */, const int32_t* offsets /* device [G + 1] */, int M, int G, int chunk,
                      int32_t* below /* [3,G,C,T] */, int32_t* inside /* [G,C,T] or NULL */, int32_t* cross /* [G,C,T] or NULL */,
                      float* pinball /* [3,G,C] or NULL */, float* width /* [G,C] or NULL */, void* scratch, size_t scratch_bytes,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- data parallel with the small payload (one collective per step) -----------------------------------------------------
 * The encoder's chain rule is linear in G = g_pre^T [X | 1] (and the head layers' gradients in glat^T [hid | 1]): a rank only has to
 * contribute its shard's G, its head-layer products and its ODE-half gradient row with the loss scalar --
 *   payload = [G: Hc x (C T + 1) | G_loc: L x (Hc + 1) | G_ls: L x (Hc + 1) | loss | gradient of flat range [ode_begin, n_params)]
 * (kind AUX: the row holds [loss | label-head range]), slode_grad_payload_floats floats (34,204 = 137 KB at BASELINE config[1] / [3]
 * against the 96,463 of [flat gradient | loss]).  One step on N ranks =
 *   slode_grad_partial (fold, [encoder,] ODE / aux kernel, split-K products, pack)  ->  SUM all-reduce of `payload` (RCCL; the caller's,
 *   torch.distributed.all_reduce in svi.py)  ->  slode_grad_apply (chain rule, final reduction, Adam) on every rank.
 * Both calls must use the SAME workspace with no other step on it in between (the fold's w' / row sums stay there).  Folded encoder
 * path only (dense [B,T,C] or [B,C,T] observations): otherwise SLODE_EINVAL, and the caller reduces the flat gradient of slode_svi_step
 * instead.  Replaces, like slode_svi_step, `losses[i].step(**d)` of training_cvs.py:152 on each rank of a data-parallel job. */
size_t slode_grad_payload_floats(const slode_shape* s, const slode_layout* lay, int kind);
int slode_grad_partial(slode_handle h, const slode_shape* s, const slode_layout* lay, int kind, const float* params, const float* times,
                       const float* stage_t, const slode_batch* batch, float* payload, void* workspace, size_t workspace_bytes, void* stream);
/* obs_strides: the batch's observation strides (they select the fold's column order).  loss_out[0] = the payload's loss slot (the global
 * -ELBO after the all-reduce); grads[0, n_params) written; adam != NULL: update applied by the same launch. */
int slode_grad_apply(slode_handle h, const slode_shape* s, const slode_layout* lay, int kind, float* params, const int64_t obs_strides[3],
                     const float* payload, float* loss_out, float* grads, void* workspace, size_t workspace_bytes, const slode_adam* adam,
                     void* stream);

/* Measured arm, OFF by default (SLODE_FOLD_NEXT=1 in the environment of slode_create turns it on): the launch that applies a step's Adam
 * update also folds the UPDATED encoder weights (W_eff & co.: csrc/encoder_fused.hip) and leaves them in the workspace, so consecutive
 * training steps on one (workspace, params) pair -- slode_svi_step / slode_elbo_adam_step / slode_aux_step / slode_grad_apply with Adam --
 * start without a fold launch.  Bitwise the same results; on MI355X the hand-offs inside the launch cost 6.0 us where the fold launch costs
 * 5.5, hence off.  When it is on, the workspace carries state from step to step and the library notices every weight change IT
 * makes; a caller that writes the parameter vector (or the workspace) itself between two steps -- checkpoint load, `load_state_dict`, its
 * own optimizer -- calls slode_fold_invalidate first.  With the arm off the call is a no-op.  The waits inside the launch are bounded: when
 * one fires, W_eff is NaN-poisoned and the next loss is NaN (one bench run of a B = 128 shape averaged 308 instead of 46 us per step --
 * profiles/r04_h_ab24_fold_next_all_configs.log); a diagnostic form, not for production runs. */
int slode_fold_invalidate(slode_handle h);

/* The handle's noise generator (replaces torch's global generator behind `rsample`): Philox-4x32-10 keyed by `seed`; the draw of
 * (drawing call n, trajectory b, latent index l) is word l & 3 -> Box-Muller of block [b + first_trajectory | l >> 2 | n] -- stateless,
 * so results do not depend on the grid or on how a global batch is sharded (data parallel: every rank passes the global index of its
 * shard's first trajectory).  slode_rng_seed resets the call counter n to 0; every step / evaluate call with eps == NULL uses the
 * current n and then increments it.  slode_rng_get reads (seed, first_trajectory, n) -- checkpoint / resume. */
int slode_rng_seed(slode_handle h, uint64_t seed, int64_t first_trajectory);
int slode_rng_set_counter(slode_handle h, uint64_t n);
int slode_rng_get(slode_handle h, uint64_t* seed, int64_t* first_trajectory, uint64_t* n);
/* The noise drawing call `n` would use for B trajectories of latent dim L, without running a step: eps_out[B, L] (NULL to skip) and the
 * raw Philox words raw_out[B, ceil(L / 4), 4] (uint32; NULL to skip).  Tests, and callers that want the explicit-eps path to reproduce
 * an in-kernel draw. */
int slode_rng_normal(slode_handle h, uint64_t n, int32_t B, int32_t L, float* eps_out, uint32_t* raw_out, void* stream);

/* torch.normal(loc, scale) of the eval-side callers (recon / classifier / pred_inputs: models/mechanistic_cvs.py:285, 300, 309):
 * z_out[B, L] = loc + scale * eps with eps from the handle's generator (one drawing call: uses the current counter n, then n + 1). */
int slode_sample_normal(slode_handle h, int32_t B, int32_t L, const float* loc, const float* scale, float* z_out, void* stream);

/* torch.optim.Adam step as pyro.optim.Adam applies it per parameter (training_cvs.py:226-227): in-place on flat
 * buffers.  step = 1-based step count. */
int slode_adam_step(slode_handle h, int64_t n, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                    float lr, float beta1, float beta2, float eps, int64_t step, void* stream);

/* Per-parameter step counts of pyro.optim.Adam (one torch.optim.Adam per parameter, state created at the first non-None gradient):
 * the two SVI objects of the reference share one optimizer (training_cvs.py:226-249) and alternate main, aux, main, ...; every
 * parameter is registered by both (pyro.module(..., self)), so all are stepped twice per minibatch -- except that the label heads of the
 * cvs / challenge families have no gradient yet in the very first main step and are skipped there.  Elements [lo, hi) of the flat
 * vector therefore use step + step_delta (skipped while that is < 1) in every Adam this handle applies (slode_adam_step,
 * slode_elbo_adam_step, slode_aux_step).  Default: empty region. */
int slode_adam_region(slode_handle h, int64_t lo, int64_t hi, int64_t step_delta);

/* Diagnostic (no reference counterpart; torchdiffeq does not report it): accepted steps per trajectory of the last adaptive (dopri5,
 * bosh3, fehlberg2, adaptive_heun) training step run on this workspace -> counts[B] (int32, device; [K * B] with K particles).  -1: 20,000 attempted steps exhausted; > capacity: record overflow (the
 * capacity is slode_dopri5_kmax: 2^26 / (B (S + 2)) steps, within [64, 2048]).  A training step in which any trajectory did either
 * returns a NaN loss and an all-NaN gradient (with Adam inside: NaN parameters), never a finite gradient that lacks that trajectory's
 * solver share; the trajectories and the forward-only loss of an overflowed step are those of the solve, which is complete. */
int slode_dopri5_step_counts(slode_handle h, const slode_shape* s, const slode_layout* lay, const void* workspace,
                             size_t workspace_bytes, int* counts, void* stream);

/* Measurement aid for bench.py's roofline block (no reference counterpart).  on = 1: every kernel that slode_elbo_step /
 * slode_elbo_adam_step / slode_aux_step / slode_adam_step / slode_eval_stats / slode_recon_moments / slode_traj_bounds / slode_label_evidence / slode_posterior_refine / slode_pointwise_density / slode_pointwise_loo / slode_intervene_moments / slode_latent_attribution / slode_curve_summary / slode_intervene_summary / slode_recon_quantiles / slode_mechanism_moments / slode_forecast_moments / slode_cohort_moments / slode_calibration / slode_joint_band launch from now on carries its own start / stop event pair (hipExtLaunchKernelGGL):
 * the begin -> end device timestamps of that dispatch -- the duration rocprofv3 --kernel-trace reports for it -- without any extra
 * packet on `stream`; on = 0: off.  slode_profile_read waits for the kernels of the LAST such call on this handle and returns their
 * number n (<= max_kernels; a negative slode_status on error), their names (static strings: "weff", "enc_fwd2", "ode_elbo", "enc_bwd_lin",
 * "enc_chain", "dopri5_fwd", "dopri5_bwd", "aux", "enc_bwd2", "slab_stage1", "reduce", "adam", "eval_stats", "eval_reduce", "recon_moments", "traj_bounds", "label_evidence", "posterior_refine", "pointwise_density", "pointwise_loo", "latent_attribution", "curve_summary", "intervene_summary", "recon_quantiles", "mechanism_moments", "intervene_moments", "forecast_moments", "forecast_summary", "cohort_plan", "cohort_moments", "cohort_merge", "calibration", "calibration_merge", "joint_band", ...) in launch order and their durations in
 * microseconds. */
#define SLODE_PROFILE_MAX_KERNELS 16
int slode_profile_enable(slode_handle h, int on);
int slode_profile_read(slode_handle h, int max_kernels, const char** names, float* us);

#ifdef __cplusplus
}
#endif
#endif /* SLODE_H */
