// Per-trajectory bounds from K latent draws (slode_traj_bounds): for every trajectory b the K per-draw losses
//   loss[k][b] = -(log-likelihood + log p(z | labels) - log q(z | x)) (+ proc's 46 x label terms),  z = loc(x_b) + scale(x_b) eps[k][b]
// -- the main loss of the single row b on draw k -- kept apart, and their four summaries: the mean (-ELBO of the trajectory), the
// importance-weighted bound -log(1/K sum_k exp(-loss)), the effective sample size of the weights, the mean negative log-likelihood.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. K - 1:
// The forward phases B0 (weights), B3-B5 (fwd_solve), the state and head values of B6, the prior nets of B1 and the logits of B7 are the
// shared ones of slode_forward.h; B1 / B2 are this kernel's own: it keeps both distributions for the KL terms.
//   B0  once per workgroup: the weights every draw reuses (fwd_stage_weights: [w_t | u_j | W_g | W_d] per hidden unit, the
//       z-columns of the hidden layer and the init net, the init net's output layer, the head weights, the biases) and the likelihood
//       scale table of the fold launch (1 / scale and log scale per (c, t)) into the LDS
//   B1  once per trajectory: labels; loc / scale of the posterior (encoder launch) and the conditional prior nets, kept in the registers
//       of thread l; the observation row into the LDS as [C][T] -- HBM is read once per trajectory, not once per draw
//   per draw:
//   B2  z = loc + scale * eps_k (row b of drawing call n + k, or of the explicit [K, B, L] tensor); log q - log p of thread l
//   B3-B5  fwd_solve over the whole grid: the init net and x0, the step table, the forward affine scan
//   B6  thread <-> time point: decoder heads + ALD / Gaussian log-likelihood against the staged observations
//   B7  proc family: the main loss's label terms on z, a half-wave per label head (as phase E5 of eval_stats_kernel, use 2)
//   B8  fixed-order sums over the workgroup of (log q - log p) and of the log-likelihood; thread 0 forms loss[k] and its likelihood part
//   B9  once per trajectory, over the K stored values, in fp64: min, sums, sum exp, sum exp^2 -> the four slots as ONE 16-byte store;
//       loss_kb with plain per-lane stores
// Every sum runs in a fixed order that depends on (K, T, L) alone: the result is a function of (parameters, inputs, noise) -- bitwise equal
// between runs, between one workgroup per trajectory and the persistent loop, between in-kernel and explicit noise.  No atomics.
// The frame (kernel arguments, LDS pieces, B0 / B1's staging), the draw loop B2 - B8 and B9 are the routines of traj_terms.h:
// label_evidence_kernel below (slode_label_evidence) executes them against V label hypotheses, pointwise_kernel.hip
// for its importance weights, refine_kernel.hip inside its iteration.
#include "traj_terms.h"

namespace {

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct TbLds { FwdLds f; ScoredLds s; int loss, nll, total; };

struct TbK {
  FwdK f;
  PriorK pr;
  LabelHeadK lh;
  ScoredK d;
  float *bounds, *loss_kb;
  TbLds o;
};

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
// LAB: the main loss scores the labels (aux_in_main: proc) -- phase B7 exists; without it the label-head code costs no registers
template <int SC, bool LAB>
__global__ void __launch_bounds__(TB_NT) traj_bounds_kernel(const TbK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_tb[];
  const FwdK& f = k.f;
  const int tid = threadIdx.x, T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C;
  const FwdSm sm = fwd_sm(s_tb, k.o.f);
  const ScoredSm ss = scored_sm(s_tb, k.o.s);
  float* s_loss = s_tb + k.o.loss; // [K] the trajectory's per-draw losses
  float* s_nll = s_tb + k.o.nll;   // [K] their negative log-likelihood parts

  // ---- B0: the weights every draw reuses; the likelihood scale table ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  tb_stage_scales(k.d, ss, C * T, tid);

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- B1 ----
    __syncthreads();   // (B0's writes; the previous trajectory's readers of s_u / s_obs / s_loss / s_nll are done)
    if (tid < k.pr.nu) sm.u[tid] = slode_label_at(k.d.lab, k.d.u, k.pr.nu, b, tid);
    tb_stage_obs<false>(k.d, ss, b, T, C, tid);
    __syncthreads();
    TbDim q;   // thread l < L keeps its latent dim's posterior and prior
    if (tid < L) tb_dim_load(q, k.d, k.pr, f.params, sm.u, b, L, tid, true);
    tb_draw_losses<SM, LAB, false>(f, k.lh, k.d, sm, ss, S, b, q, s_loss, s_nll, tid);   // B2 - B8
    // ---- B9: the K stored values -> the four slots and loss_kb ----
    __syncthreads();
    tb_reduce_draws(s_loss, s_nll, ss.dred, k.d.nd, f.B, b, k.bounds + (long long)b * SLODE_BOUND_SLOTS, k.loss_kb, nullptr);
  }
}

TbLds tb_lds(const slode_shape& s, int nd, bool generic) {
  LdsCarve cv;
  TbLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.s = scored_lds(cv, s, false, SLODE_MAX_AUX, 24);
  // the K losses and their likelihood parts come last; a K that cannot fit anyway counts as the whole budget (no overflow of the offsets)
  const int kd = nd < SLODE_TRAJ_BOUNDS_LDS_MAX / 4 ? nd : SLODE_TRAJ_BOUNDS_LDS_MAX / 4;
  o.loss = cv.take(kd); o.nll = cv.take(kd);
  o.total = cv.n;
  return o;
}

// ---- label evidence (slode_label_evidence): V label hypotheses scored on the K posterior draws of every trajectory ----------------------
// loss[v][k][b] = the main loss of row b on draw k with its labels replaced by hypothesis v -- what traj_bounds_kernel gives for that label
// set on the same noise, bit for bit -- and per (b, v): the mean, the importance-weighted bound, the ESS, the log-posterior over v.
// The draws z_k ~ q(z | x_b), the solve, the heads, the likelihood and (proc) the label logits do not depend on the hypothesis; only
// log p(z | u_v) and the label log-probabilities do.  One workgroup per trajectory (persistent loop beyond the grid), as traj_bounds_kernel:
//   E0  = B0
//   E1  once per trajectory: the V label rows u_v (the trajectory's own row with the columns of every hypothesised tensor replaced by row v
//       of that tensor) into the LDS; the observation row; loc / scale of the posterior in the registers of lane l of EVERY wave; the V prior
//       rows (ploc, pls, exp(-pls))[v][l] from fwd_prior_at on the staged u_v into the LDS
//   per draw:
//   E2  z = loc + scale * eps_k (B2's z); E3-E5 fwd_solve; E6 tb_loglik_points -- once
//   E7  (LAB) the logits of the label heads once (fwd_label_logits, every lane then takes the bits of lane 0 of its half-wave: the lane
//       traj_bounds_kernel stores from); lane j of the head's half-wave scores hypotheses j, j + 32 with tb_label_logprob against u_v
//   E8  wave w takes the hypotheses v = w, w + 4, ...: lane l < L forms tb_logq_minus_logp against prior row v, wave_sum; the wave sums of
//       the likelihood; then thread v forms loss[v][k]
//   E9  per hypothesis tb_reduce_draws on its K losses (slots 0-2 and the fp64 bound into the LDS, loss_vkb[v] to memory), then thread 0
//       forms the V log-posteriors and the arg-max in fp64 (le_posterior); thread v stores row (b, v) as ONE 16-byte store
// Why column v has the bits of traj_bounds_kernel on label set v.  L <= SLODE_MAX_L = 64, so in traj_bounds_kernel every latent dim lives in
// wave 0: the (log q - log p) partials of waves 1-3 are wave sums of +0 = +0, and its tree gives kl = (w0 + 0) + (0 + 0).  Here wave w
// computes the same lanes' terms with the same routine from the same values (z read back from the LDS, loc / scale loaded by every wave,
// the prior row formed by the same fwd_prior_at / expf) and the same wave_sum -- the bits of w0 -- and thread v adds the same three zeros.
// The likelihood sums are the same code on the same draw.  The label terms come from the same logits (lane 0's) and tb_label_logprob, a
// routine without cross-lane operations, so which lane runs it does not matter.  loss = kl - ll + items in the same order, and the K
// losses go through the same tb_reduce_draws.  No atomics; every sum in a fixed order that depends on (K, V, T, L) alone.
struct LeLds { FwdLds f; ScoredLds s; int nll, uh, prior, kl, ev, bd, loss, total; };   // (s.item: [V][SLODE_MAX_AUX])

struct LeK {
  FwdK f;
  PriorK pr;
  LabelHeadK lh;
  ScoredK d;
  int nv;
  const float* log_prior;
  float *evidence, *loss_vkb;
  int32_t* best;
  LeLds o;
  LabelSrc hyp;   // hyp.p[i] == nullptr: label tensor i is not hypothesised (widths and offsets: d.lab's)
};

// column col of label row u_v of trajectory b
__device__ __forceinline__ float le_label_at(const LabelSrc& hyp, const LabelSrc& ls, long long b, int v, int col) {
  int i = 0;
#pragma unroll
  for (int q = 1; q < SLODE_MAX_LABELS; ++q) i = (q < ls.n && col >= ls.off[q]) ? q : i;
  const int w = ls.off[i + 1] - ls.off[i], c = col - ls.off[i];
  const float* hp = hyp.p[i];
  return hp ? hp[(long long)v * w + c] : ls.p[i][b * w + c];
}

// E9, thread 0 alone: log_post[v] = t_v - logsumexp_v'(t_v'), t_v = log_prior[v] - bound[v], in fp64 from the unrounded bounds, in the
// order v = 0 .. V - 1 (V = 1: t - (t + log(exp(0))) = 0 exactly) into slot 3 of the staged rows; the arg-max, the lowest index on a tie.
// Not inlined, for the reason of tb_reduce_draws.
__device__ __noinline__ void le_posterior(const double* s_bd, const float* __restrict__ log_prior, int V, float* s_ev, int32_t* best) {
  double m = -1.0 / 0.0;
  for (int v = 0; v < V; ++v) m = fmax(m, (log_prior ? (double)log_prior[v] : 0.0) - s_bd[v]);
  double se = 0.0;
  for (int v = 0; v < V; ++v) se += exp(((log_prior ? (double)log_prior[v] : 0.0) - s_bd[v]) - m);
  const double lse = m + log(se);
  double bv = -1.0 / 0.0;
  int bi = 0;
  for (int v = 0; v < V; ++v) {
    const double p = ((log_prior ? (double)log_prior[v] : 0.0) - s_bd[v]) - lse;
    s_ev[4 * v + 3] = (float)p;
    if (p > bv) { bv = p; bi = v; }
  }
  if (best) *best = bi;
}

template <int SC, bool LAB>
__global__ void __launch_bounds__(TB_NT) label_evidence_kernel(const LeK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_tb[];
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = tid >> 5, j32 = tid & 31;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, Q = f.Q, nd = k.d.nd, V = k.nv, nu = k.pr.nu;
  const FwdSm sm = fwd_sm(s_tb, k.o.f);
  const ScoredSm ss = scored_sm(s_tb, k.o.s);
  float* s_red = ss.red;             // [4 .. 8) per-wave sums of the log-likelihood
  float* s_nll = s_tb + k.o.nll;     // [K] the draws' negative log-likelihood (the same for every hypothesis)
  float* s_uh = s_tb + k.o.uh;       // [V][nu] the label rows u_v
  float* s_pr = s_tb + k.o.prior;    // [V][3][L] ploc | pls | exp(-pls)
  float* s_kl = s_tb + k.o.kl;       // [V] sum over l of (log q - log p_v) of the draw
  float* s_item = ss.item;           // [V][SLODE_MAX_AUX] -46 x label log-prob of the draw against u_v, per head
  float* s_ev = s_tb + k.o.ev;       // [V][4] the rows of the trajectory before their store
  float* s_loss = s_tb + k.o.loss;   // [V][K] the per-draw losses
  double* s_bd = reinterpret_cast<double*>(s_tb + k.o.bd);       // [V] the importance-weighted bounds before they are rounded
  const int n_items = LAB ? k.lh.n_aux : 0;

  // ---- E0 ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  tb_stage_scales(k.d, ss, C * T, tid);

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- E1 ----
    __syncthreads();   // (E0's writes; the previous trajectory's readers of every table are done)
    for (int i = tid; i < V * nu; i += TB_NT) { const int v = i / nu; s_uh[i] = le_label_at(k.hyp, k.d.lab, b, v, i - v * nu); }
    {   // (tb_stage_obs<false>, written out: as a routine it costs this kernel three VGPRs, and <5, -> would fall from 4 waves per SIMD to 3)
      const float* ob = k.d.obs + (long long)b * k.d.sb;
      for (int i = tid; i < C * T; i += TB_NT) {
        int c, t;
        if (k.d.t_major) { t = i / C; c = i - t * C; } else { c = i / T; t = i - c * T; }
        ss.obs[c * T + t] = ob[i];
      }
    }
    __syncthreads();
    float loc = 0.f, sc = 1.f, nlsc = 0.f;   // lane l < L of every wave keeps its latent dim's posterior
    if (lane < L) { loc = k.d.loc[(long long)b * L + lane]; sc = k.d.scale[(long long)b * L + lane]; nlsc = -logf(sc); }
    for (int i = tid; i < V * L; i += TB_NT) {   // (read after the draw's first barrier)
      const int v = i / L, l = i - v * L;
      float pl, pls;
      fwd_prior_at(k.pr, par, s_uh + v * nu, l, pl, pls);
      s_pr[(v * 3) * L + l] = pl; s_pr[(v * 3 + 1) * L + l] = pls; s_pr[(v * 3 + 2) * L + l] = expf(-pls);
    }
    for (int kk = 0; kk < nd; ++kk) {
      // ---- E2 ----
      if (tid < L) sm.z[tid] = fmaf(sc, slode_eps_at(k.d.rng, k.d.eps, b, L, tid, kk, f.B), loc);
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] / s_item / s_kl / s_red are done)
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // E3 - E5
      // ---- E6 ----
      const float llt0 = tb_loglik_points<SM>(sm, S, T, C, Q, k.d.gauss, k.d.tau, ss.obs, ss.inv, ss.lg, tid);
      // ---- E7 ----
      if (LAB) {   // (every lane of a wave takes part in every sum)
        const bool on = hw < n_items;
        const int a = on ? hw : 0;
        const slode_aux ax = k.lh.aux[a];
        float lg[8];
        fwd_label_logits(k.lh, par, a, sm.z + ax.z_off, j32, lg);
#pragma unroll
        for (int q = 0; q < 8; ++q) lg[q] = __shfl(lg[q], lane & 32, 64);
        for (int v = j32; v < V; v += 32) {
          const float lp = tb_label_logprob(k.lh, par, a, lg, s_uh + v * nu + ax.u_off);
          if (on) s_item[v * SLODE_MAX_AUX + a] = -k.lh.aux_mult * lp;
        }
      }
      // ---- E8 ----
      const float z = lane < L ? sm.z[lane] : 0.f;
      for (int v = wave; v < V; v += TB_NT / 64) {   // (wave-uniform)
        float klt = 0.f;
        if (lane < L) klt = tb_logq_minus_logp(z, loc, sc, nlsc, s_pr[(v * 3) * L + lane], s_pr[(v * 3 + 1) * L + lane], s_pr[(v * 3 + 2) * L + lane]);
        klt = wave_sum(klt);
        if (lane == 0) s_kl[v] = klt;
      }
      const float llt = wave_sum(llt0);
      if (lane == 0) s_red[4 + wave] = llt;
      __syncthreads();
      if (tid < V) {
        const float kl = (s_kl[tid] + 0.f) + (0.f + 0.f), ll = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);   // (the tree of B8: header)
        float loss = kl - ll;
        for (int a = 0; a < n_items; ++a) loss += s_item[tid * SLODE_MAX_AUX + a];
        s_loss[tid * nd + kk] = loss;
        if (tid == 0) s_nll[kk] = -ll;
      }
    }
    // ---- E9 ----
    for (int v = 0; v < V; ++v) {
      __syncthreads();   // (the draws' writes; the previous hypothesis' readers of s_dred are done)
      tb_reduce_draws(s_loss + v * nd, s_nll, ss.dred, nd, f.B, b, s_ev + 4 * v, k.loss_vkb ? k.loss_vkb + (long long)v * nd * f.B : nullptr, s_bd + v);
    }
    __syncthreads();
    if (tid == 0) le_posterior(s_bd, k.log_prior, V, s_ev, k.best ? k.best + b : nullptr);
    __syncthreads();
    if (tid < V) {
      typedef float f4_t __attribute__((ext_vector_type(4)));
      reinterpret_cast<f4_t*>(k.evidence)[(long long)b * V + tid] = reinterpret_cast<const f4_t*>(s_ev)[tid];   // one 16-byte store
    }
  }
}

LeLds le_lds(const slode_shape& s, int nd, int V, bool generic) {
  const int cap = SLODE_LABEL_EVIDENCE_LDS_MAX / 4;
  LdsCarve cv;
  LeLds o{};
  o.f = fwd_lds(cv, s, generic);
  const int vv = V < 1 ? 1 : (V > SLODE_EVIDENCE_MAX_V ? SLODE_EVIDENCE_MAX_V : V);
  o.s = scored_lds(cv, s, false, vv * SLODE_MAX_AUX, 24);
  o.uh = cv.take(vv * (s.n_u > 0 ? s.n_u : 1)); o.prior = cv.take(vv * 3 * s.L); o.kl = cv.take(vv);
  o.ev = cv.take(vv * 4); o.bd = cv.take(vv * 2);
  // the K likelihood parts and the V x K losses come last; sizes that cannot fit anyway count as the whole budget (no overflow of the offsets)
  const long long kv = (long long)vv * (nd < 0 ? 0 : nd);
  o.nll = cv.take(nd < cap ? (nd < 0 ? 0 : nd) : cap); o.loss = cv.take(kv < cap ? (int)kv : cap);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_traj_bounds_lds_bytes(const slode_shape& s, int num_draws, int force_generic) {
  return (size_t)tb_lds(s, num_draws, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_traj_bounds(const TrajBoundsLaunch& a, hipStream_t stream) {
  const ScoredLaunch& d = a.d;
  const slode_shape& s = d.s;
  TbK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay); fwd_fill(k.lh, s, d.lay); fwd_fill(k.d, d);
  k.bounds = a.bounds; k.loss_kb = a.loss_kb;
  k.o = tb_lds(s, d.num_draws, fwd_generic(s, d.force_generic));
  const size_t lds = slode_traj_bounds_lds_bytes(s, d.num_draws, d.force_generic);
  if (lds > SLODE_TRAJ_BOUNDS_LDS_MAX || d.num_draws < 1 || d.grid < 1 || s.n_aux > SLODE_MAX_AUX) return hipErrorInvalidValue;
  const bool lab = s.aux_in_main && s.n_aux > 0;
  fwd_dispatch(s, d.force_generic, [&](auto sc) {
    constexpr int SC = decltype(sc)::value;
    if (lab) fwd_launch("traj_bounds", traj_bounds_kernel<SC, true>, d.grid, lds, stream, k);
    else fwd_launch("traj_bounds", traj_bounds_kernel<SC, false>, d.grid, lds, stream, k);
  });
  return hipGetLastError();
}

size_t slode_label_evidence_lds_bytes(const slode_shape& s, int num_draws, int V, int force_generic) {
  return (size_t)le_lds(s, num_draws, V, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_label_evidence(const LabelEvidenceLaunch& a, hipStream_t stream) {
  const ScoredLaunch& d = a.d;
  const slode_shape& s = d.s;
  LeK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay); fwd_fill(k.lh, s, d.lay); fwd_fill(k.d, d);
  k.nv = a.V; k.log_prior = a.log_prior; k.evidence = a.evidence; k.loss_vkb = a.loss_vkb; k.best = a.best; k.hyp = a.hyp;
  k.o = le_lds(s, d.num_draws, a.V, fwd_generic(s, d.force_generic));
  const size_t lds = slode_label_evidence_lds_bytes(s, d.num_draws, a.V, d.force_generic);
  if (lds > SLODE_LABEL_EVIDENCE_LDS_MAX || d.num_draws < 1 || a.V < 1 || a.V > SLODE_EVIDENCE_MAX_V || d.grid < 1 || s.n_aux > SLODE_MAX_AUX ||
      d.lab.n < 1)
    return hipErrorInvalidValue;
  const bool lab = s.aux_in_main && s.n_aux > 0;
  fwd_dispatch(s, d.force_generic, [&](auto sc) {
    constexpr int SC = decltype(sc)::value;
    if (lab) fwd_launch("label_evidence", label_evidence_kernel<SC, true>, d.grid, lds, stream, k);
    else fwd_launch("label_evidence", label_evidence_kernel<SC, false>, d.grid, lds, stream, k);
  });
  return hipGetLastError();
}
