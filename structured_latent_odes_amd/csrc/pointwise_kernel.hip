// Pointwise predictive density from K latent draws (slode_pointwise_density): for every trajectory b and observation point i = (c, t), with
//   l_k[i] = sum over the Q heads of the log-likelihood terms of that point on draw k (the addends of tb_loglik_points for channel c at time t)
// and normalised draw weights w_k = exp(lw_k), the three planes
//   lppd[i] = log sum_k w_k exp(l_k[i]),   mean_ll[i] = sum_k w_k l_k[i],   var_ll[i] = sum_k w_k (l_k[i] - mean_ll[i])^2
// and eight sums per trajectory (SLODE_POINTWISE_SLOTS: the planes over the points inside / outside the mask, the counts, the ESS).
// Weights: posterior (w_k = 1 / K, one sweep over the draws, no KL term) or importance (w_k ~ exp(-loss_k), loss_k the per-draw loss of
// traj_bounds_kernel with the mask on its likelihood terms: sweep 1 IS that kernel's loop B2 - B8, then the weights, then sweep 2 redraws the
// same counter-based noise -- the same z bit for bit -- solves again and folds the points with the final weights).
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid), the frame of traj_bounds_kernel:
//   P0  = B0: staged weights, the likelihood scale table
//   P1  once per trajectory: labels, observations and mask weights [C][T] (mask == NULL: all 1); posterior and prior of thread l
//   importance mode:  P2 - P8 = tb_draw_losses, traj_bounds_kernel's draw loop with the weighted log-likelihood (refine_kernel's R4: at
//       weight 1 the sum of B6) -> s_loss[k]; then tb_reduce_draws (loss_kb, the ESS, the fp64 bound) and pw_weights:
//       lw_k = (bound - log K) - loss_k in fp64 -> lw_k rounded to fp32 and w_k = exp(lw_k) kept in fp64
//   per draw:  P9 z (the same noise rows), fwd_solve, the point fold: thread <-> time point t = tid, tid + 256, ...; for each of its C channels
//       the thread alone owns the point's accumulators in the LDS tables [.][C][T]: running maximum M and sum s of a_k = lw_k + l_k (draw 0:
//       M = a_0, s = 1), the shift l_0 and the fp64 shifted sums S1 += w d, S2 += w d^2 of d = l_k - l_0
//   P10 once per trajectory: lppd = M + log s, mean_ll = l_0 + S1, var_ll = max(S2 - S1^2, 0), stored along T (coalesced); the summary from the
//       ROUNDED plane values in fp64: the thread's points in the order (t, c), tb_wave_sum_d, the four waves as (0 + 1) + (2 + 3); two
//       16-byte stores
// At K = 1: lw_0 = 0 and w_0 = 1 exactly, so lppd == mean_ll == l_0 bit for bit and var_ll == 0.  The shifted sums are kept in fp64 (and
// the weights with them): with weights that collapse onto one draw j != 0, S2 - S1^2 = w_j (1 - w_j) d_j^2 cancels to the rounding of
// w_j, and an fp32 w_j would leave 3e-8 d_j^2 where the true variance is ~0.
// Every sum runs in a fixed order that depends on (K, C, T, L) alone: every output is a function of (parameters, inputs, mask, posterior,
// noise) -- bitwise equal between runs, between grids, between in-kernel and explicit noise.  No atomics.
#include "traj_terms.h"

namespace {

constexpr int PW_NT = FWD_NT;
constexpr int PW_SUMS = 7;   // fp64 sums of the summary: slots 0 - 6

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct PwLds { FwdLds f; ScoredLds s; int row, bd, sum, pm, ps, p0, s1, s2, loss, nll, lw, wt, total; };

struct PwK {
  FwdK f;
  PriorK pr;
  LabelHeadK lh;
  ScoredK d;
  int imp;
  float lw_u;    // posterior mode: -log K (K = 1: +0)
  double w_u;    //                 1 / K
  float *point, *summary, *loss_kb;
  PwLds o;
};

// the point fold of one draw: l_k[i] of the thread's points (the addends of tb_loglik_points, summed over the heads of one channel) into the
// accumulators of point i = c T + t, which this thread alone reads and writes.  lw / wt: the draw's log-weight (fp32) and weight (fp64).
template <int SM>
__device__ __forceinline__ void pw_fold_points(const FwdSm& sm, int S, int T, int C, int Q, int gauss, const float (&tau)[3], const float* s_obs,
                                               const float* s_inv, const float* s_lg, float* s_pm, float* s_ps, float* s_p0, double* s_s1,
                                               double* s_s2, bool first, float lw, double wt, int tid) {
  for (int t = tid; t < T; t += PW_NT) {
    float x[SM];
    fwd_state_at<SM>(sm, S, t, x);
    for (int c = 0; c < C; ++c) {
      const int i = c * T + t;
      const float obv = s_obs[i], inv = s_inv[i], lg = s_lg[i];
      const float l = tb_point_loglik<SM>(sm, S, C, Q, c, gauss, tau, obv, inv, lg, x);
      const float a = lw + l;
      if (first) { s_pm[i] = a; s_ps[i] = 1.f; s_p0[i] = l; s_s1[i] = 0.0; s_s2[i] = 0.0; }
      else {
        const float m = s_pm[i];
        if (a > m) { s_ps[i] = fmaf(s_ps[i], expf(m - a), 1.f); s_pm[i] = a; }
        else s_ps[i] += expf(a - m);
        const double d = (double)l - (double)s_p0[i], wd = wt * d;   // (exact: an fp32 difference would round at |l - l_0|, which a bad draw 0 makes large)
        s_s1[i] += wd; s_s2[i] = fma(wd, d, s_s2[i]);
      }
    }
  }
}

// importance mode, after tb_reduce_draws: lw_k = -loss_k - logsumexp_j(-loss_j) = (bound - log K) - loss_k in fp64 (bound: the unrounded
// importance-weighted bound of tb_reduce_draws; K = 1: bound = loss_0 and log 1 = 0, so lw_0 = 0 and w_0 = 1 exactly).  Not inlined, for
// the reason of tb_reduce_draws.
__device__ __noinline__ void pw_weights(const float* s_loss, const double* s_bd, int nd, float* s_lw, double* s_wt) {
  const double lz = *s_bd - log((double)nd);
  for (int q = threadIdx.x; q < nd; q += PW_NT) {
    const double lw = lz - (double)s_loss[q];
    s_lw[q] = (float)lw; s_wt[q] = exp(lw);
  }
}

// P10: the planes of the thread's points and its part of the summary; then the fixed tree.  Not inlined: the fp64 partials and the logf
// constants stay out of the draw loops' register budget.
__device__ __noinline__ void pw_finish(const float* s_pm, const float* s_ps, const float* s_p0, const double* s_s1, const double* s_s2,
                                       const float* s_w, double* s_sum, int T, int C, long long B, long long b, float ess,
                                       float* __restrict__ point, float* __restrict__ summary) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long plane = B * C * T;
  double acc[PW_SUMS];
#pragma unroll
  for (int j = 0; j < PW_SUMS; ++j) acc[j] = 0.0;
  for (int t = tid; t < T; t += PW_NT)
    for (int c = 0; c < C; ++c) {
      const int i = c * T + t;
      const double s1 = s_s1[i];
      const float lppd = s_pm[i] + logf(s_ps[i]);
      const float mean = (float)((double)s_p0[i] + s1);
      const float var = (float)fmax(s_s2[i] - s1 * s1, 0.0);
      const long long o = (b * C + c) * T + t;
      point[o] = lppd; point[plane + o] = mean; point[2 * plane + o] = var;
      if (s_w[i] > 0.f) { acc[0] += (double)lppd; acc[1] += (double)var; acc[2] += (double)mean; acc[3] += 1.0; }
      else { acc[4] += (double)lppd; acc[5] += (double)mean; acc[6] += 1.0; }
    }
#pragma unroll
  for (int j = 0; j < PW_SUMS; ++j) acc[j] = tb_wave_sum_d(acc[j]);
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < PW_SUMS; ++j) s_sum[wave * 8 + j] = acc[j];
  }
  __syncthreads();
  if (tid == 0) {
    typedef float f4_t __attribute__((ext_vector_type(4)));
    float o[8];
#pragma unroll
    for (int j = 0; j < PW_SUMS; ++j) o[j] = (float)((s_sum[j] + s_sum[8 + j]) + (s_sum[16 + j] + s_sum[24 + j]));
    o[7] = ess;
    f4_t lo, hi;
    lo.x = o[0]; lo.y = o[1]; lo.z = o[2]; lo.w = o[3]; hi.x = o[4]; hi.y = o[5]; hi.z = o[6]; hi.w = o[7];
    f4_t* row = reinterpret_cast<f4_t*>(summary + b * SLODE_POINTWISE_SLOTS);
    row[0] = lo; row[1] = hi;   // the row's eight slots: two 16-byte stores
  }
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
// LAB: the main loss scores the labels (aux_in_main: proc) -- phase P7 exists (importance mode)
template <int SC, bool LAB>
__global__ void __launch_bounds__(PW_NT) pointwise_kernel(const PwK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_pw[];
  const FwdK& f = k.f;
  const int tid = threadIdx.x, T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, Q = f.Q, nd = k.d.nd;
  const FwdSm sm = fwd_sm(s_pw, k.o.f);
  const ScoredSm ss = scored_sm(s_pw, k.o.s);
  float* s_row = s_pw + k.o.row;   // [4] the four slots of tb_reduce_draws (slot 2: the ESS)
  float* s_pm = s_pw + k.o.pm;     // [C][T] running maximum of a_k
  float* s_ps = s_pw + k.o.ps;     // [C][T] sum of exp(a_k - M)
  float* s_p0 = s_pw + k.o.p0;     // [C][T] l_0, the shift
  float* s_loss = s_pw + k.o.loss; // [K] the per-draw losses          (importance mode; the four K-tables are not carved otherwise)
  float* s_nll = s_pw + k.o.nll;   // [K] their negative log-likelihood parts
  float* s_lw = s_pw + k.o.lw;     // [K] the log-weights
  double* s_bd = reinterpret_cast<double*>(s_pw + k.o.bd);       // [1] the importance-weighted bound before it is rounded
  double* s_sum = reinterpret_cast<double*>(s_pw + k.o.sum);     // [4][8] per-wave partials of the summary
  double* s_s1 = reinterpret_cast<double*>(s_pw + k.o.s1);       // [C][T] sum of w d
  double* s_s2 = reinterpret_cast<double*>(s_pw + k.o.s2);       // [C][T] sum of w d^2
  double* s_wt = reinterpret_cast<double*>(s_pw + k.o.wt);       // [K] the weights
  const bool imp = k.imp != 0;

  // ---- P0 ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  tb_stage_scales(k.d, ss, C * T, tid);

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- P1 ----
    __syncthreads();   // (P0's writes; the previous trajectory's readers of every table are done)
    if (tid < k.pr.nu) sm.u[tid] = slode_label_at(k.d.lab, k.d.u, k.pr.nu, b, tid);
    tb_stage_obs<true>(k.d, ss, b, T, C, tid);
    __syncthreads();
    TbDim q;   // thread l < L keeps its latent dim's posterior and (importance mode) prior
    if (tid < L) tb_dim_load(q, k.d, k.pr, f.params, sm.u, b, L, tid, imp);
    float ess = (float)nd;
    if (imp) {   // (workgroup-uniform)
      tb_draw_losses<SM, LAB, true>(f, k.lh, k.d, sm, ss, S, b, q, s_loss, s_nll, tid);   // P2 - P8
      __syncthreads();
      tb_reduce_draws(s_loss, s_nll, ss.dred, nd, f.B, b, s_row, k.loss_kb, s_bd);
      __syncthreads();
      pw_weights(s_loss, s_bd, nd, s_lw, s_wt);
      ess = s_row[2];
    }
    // ---- P9: the draws again (importance) or for the first time (posterior), folded per point ----
    for (int kk = 0; kk < nd; ++kk) {
      if (tid < L) sm.z[tid] = fmaf(q.sc, slode_eps_at(k.d.rng, k.d.eps, b, L, tid, kk, f.B), q.loc);
      __syncthreads();   // (also: pw_weights' writes; the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);
      const float lw = imp ? s_lw[kk] : k.lw_u;
      const double wt = imp ? s_wt[kk] : k.w_u;
      pw_fold_points<SM>(sm, S, T, C, Q, k.d.gauss, k.d.tau, ss.obs, ss.inv, ss.lg, s_pm, s_ps, s_p0, s_s1, s_s2, kk == 0, lw, wt, tid);
    }
    // ---- P10 ----
    pw_finish(s_pm, s_ps, s_p0, s_s1, s_s2, ss.w, s_sum, T, C, f.B, b, ess, k.point, k.summary);
  }
}

PwLds pw_lds(const slode_shape& s, int nd, int imp, bool generic) {
  const int CT = s.C * s.T;
  LdsCarve cv;
  PwLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.s = scored_lds(cv, s, true, SLODE_MAX_AUX, 24);
  o.row = cv.take(4); o.bd = cv.take(2); o.sum = cv.take(64);
  o.pm = cv.take(CT); o.ps = cv.take(CT); o.p0 = cv.take(CT); o.s1 = cv.take(2 * CT); o.s2 = cv.take(2 * CT);
  // importance mode: the K losses, their likelihood parts, the log-weights and the fp64 weights come last; a K that cannot fit anyway
  // counts as the whole budget (no overflow of the offsets)
  const int kd = !imp ? 0 : (nd < 0 ? 0 : (nd < SLODE_POINTWISE_LDS_MAX / 4 ? nd : SLODE_POINTWISE_LDS_MAX / 4));
  o.loss = cv.take(kd); o.nll = cv.take(kd); o.lw = cv.take(kd); o.wt = cv.take(2 * kd);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_pointwise_lds_bytes(const slode_shape& s, int num_draws, int weights, int force_generic) {
  return (size_t)pw_lds(s, num_draws, weights, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_pointwise(const PointwiseLaunch& a, hipStream_t stream) {
  const ScoredLaunch& d = a.d;
  const slode_shape& s = d.s;
  PwK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay); fwd_fill(k.lh, s, d.lay); fwd_fill(k.d, d);
  k.imp = a.weights == SLODE_PW_IMPORTANCE ? 1 : 0;
  const size_t lds = slode_pointwise_lds_bytes(s, d.num_draws, k.imp, d.force_generic);
  if (lds > SLODE_POINTWISE_LDS_MAX || d.num_draws < 1 || d.grid < 1 || s.n_aux > SLODE_MAX_AUX) return hipErrorInvalidValue;
  k.lw_u = (float)(0.0 - log((double)d.num_draws)); k.w_u = 1.0 / (double)d.num_draws;
  k.point = a.point; k.summary = a.summary; k.loss_kb = k.imp ? a.loss_kb : nullptr;
  k.o = pw_lds(s, d.num_draws, k.imp, fwd_generic(s, d.force_generic));
  const bool lab = k.imp && s.aux_in_main && s.n_aux > 0;
  fwd_dispatch(s, d.force_generic, [&](auto sc) {
    constexpr int SC = decltype(sc)::value;
    if (lab) fwd_launch("pointwise_density", pointwise_kernel<SC, true>, d.grid, lds, stream, k);
    else fwd_launch("pointwise_density", pointwise_kernel<SC, false>, d.grid, lds, stream, k);
  });
  return hipGetLastError();
}
