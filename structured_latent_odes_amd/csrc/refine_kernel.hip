// Posterior refinement (slode_posterior_refine): every trajectory b takes J Adam steps on its own phi = (loc[L], rho[L]), scale = exp(rho),
// against its own K-draw -ELBO
//   F(phi) = 1/K sum_k loss_k,   loss_k = -(sum_{c,t,q} w[b][c][t] ll_{c,t,q} + log p(z_k | u) - log q(z_k)),   z_k = loc + exp(rho) eps_k
// -- the per-draw loss of traj_bounds_kernel with a weight w >= 0 on every likelihood term -- on noise rows eps_k that are fixed for the whole
// call (F is a deterministic function), starting from the encoder launch's (loc, log scale); the best iterate over j = 0 .. J is returned.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid); weights, observations and every table stay in
// the LDS for the whole iteration.  The forward phases are the shared ones of slode_forward.h; the backward pass is this kernel's:
//   R0  once per workgroup: fwd_stage_weights; the likelihood scale table (1 / scale, log scale per (c, t))
//   R1  once per trajectory: labels, observations and weights [C][T] (mask == NULL: all 1); phi_0 and the prior of thread l
//   per iteration j = 0 .. J, per draw k:
//   R2  z = loc + scale eps_k; log q - log p of thread l
//   R3  fwd_init_state, the step table; the step coefficients A are copied aside (the scan overwrites them with the states); the forward scan
//   R4  thread <-> time point: heads, weighted log-likelihood and (backward) g_x[t][s] = -sum_{c,q} w dll/dmu hw[qc][s]
//   R5  fixed-order sums over the workgroup -> loss_k
//   backward (j < J, or j == 0 when grad0 is asked for):
//   R6  reverse affine scan lambda_n = g_n + A_n lambda_{n+1}, in place over g_x (rf_rev_scan: fwd_scan on the reversed index)
//   R7  thread <-> step: gA = lambda_{n+1} x_n, gb = lambda_{n+1}; a, d of the step's stages re-evaluated (fwd_ad); step_bwd (fixed_step.h) -> ga[r], gd[r];
//       g_pre_a = ga a (1 - a), g_pre_d = gd d (1 - d) into the table [steps x stages][2 S]
//   R8  thread <-> (hidden unit j, chunk): sum over the chunk's samples of [h_j > 0] sum_s (g_pre_a W_g + g_pre_d W_d); per-chunk partials
//   R9  thread j: g_u[j], the chunks in order; thread H + j: the init net's hidden unit from g_o = lambda_0 x0 (1 - x0)
//   R10 thread l: g_z = W_h^T g_u + W_1^T g_h0; + (z - pl) ips^2 of -log p; g_loc += g_z, g_rho += g_z scale eps - 1
//   after the K draws: F_j (the K losses summed in order in fp64), the best iterate (lowest j on a tie), one Adam step kept by thread l (in fp64).
// Every sum runs in a fixed order that depends on (K, J, T, L, H) alone: the result is a function of (parameters, inputs, noise) -- bitwise
// equal between runs, between one workgroup per trajectory and the persistent loop, between in-kernel and explicit noise.  No atomics.
#include "traj_terms.h"

namespace {

constexpr int RF_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct RfLds { FwdLds f; ScoredLds s; int ak, g, tab, part, gu, loss, fj, total; };   // (s: no item, no dred)

struct RfK {
  FwdK f;
  PriorK pr;
  ScoredK d;
  int nj;
  float lr;
  float *loc_out, *scale_out, *elbo_out, *grad0_out, *trace_out;
  int32_t* best_step;
  RfLds o;
};

// R6: lambda_n = g_n + A_n lambda_{n+1} for n = NS - 1 .. 0 (lambda_NS = g_NS), in place over g [NS + 1][S]; ak: the step coefficients [NS][S].
// fwd_scan on the reversed index m = NS - 1 - n: one state component per wave pass, a chunk of steps per lane, Kogge-Stone over the lanes' maps.
// Call with whole waves.
__device__ __forceinline__ void rf_rev_scan(float* g, const float* ak, int S, int NS, int lane, int s_first, int s_stride) {
  const int chunk = (NS + 63) / 64, m0 = min(lane * chunk, NS), m1 = min(m0 + chunk, NS);
  for (int s = s_first; s < S; s += s_stride) {
    float Ac = 1.f, bc = 0.f;   // the lane's chunk as one map
    for (int m = m0; m < m1; ++m) { const int n = NS - 1 - m; const float An = ak[n * S + s]; bc = fmaf(An, bc, g[n * S + s]); Ac *= An; }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const float Ap = __shfl_up(Ac, off, 64), bp = __shfl_up(bc, off, 64);
      if (lane >= off) { bc = fmaf(Ac, bp, bc); Ac *= Ap; }
    }
    float Ae = __shfl_up(Ac, 1, 64), be = __shfl_up(bc, 1, 64);
    if (lane == 0) { Ae = 1.f; be = 0.f; }
    float x = fmaf(Ae, g[NS * S + s], be);
    for (int m = m0; m < m1; ++m) { const int n = NS - 1 - m; x = fmaf(ak[n * S + s], x, g[n * S + s]); g[n * S + s] = x; }
  }
}

// R7: the reverse of the step table, thread <-> step: g_pre_a, g_pre_d of the nst stages of step n into tab[(n nst + r) 2 S + (s | S + s)]
template <int SM>
__device__ __forceinline__ void rf_step_table_bwd(const FwdK& k, const FwdSm& sm, int S, int nst, const float* s_g, float* s_tab, int tid) {
  const int T = k.T, H = k.H;
  for (int n = tid; n < T - 1; n += RF_NT) {
    const float h = k.times[n + 1] - k.times[n];
    const float* st = k.stage_t + (long long)n * k.R;
    float a[4][SM], d[4][SM];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (r < nst) fwd_ad<SM>(sm.row, sm.bgd, H, st[r], S, a[r], d[r]);
      else {
#pragma unroll
        for (int s = 0; s < SM; ++s) { a[r][s] = 0.f; d[r][s] = 0.f; }
      }
    }
    float x[SM];
    fwd_state_at<SM>(sm, S, n, x);
    float* row = s_tab + (long long)n * nst * 2 * S;
#pragma unroll
    for (int s = 0; s < SM; ++s) {
      if (s < S) {
        const float lam = s_g[(n + 1) * S + s];
        const float as[4] = {a[0][s], a[1][s], a[2][s], a[3][s]}, ds[4] = {d[0][s], d[1][s], d[2][s], d[3][s]};
        float ga[4], gd[4];
        step_bwd(k.method, h, as, ds, lam * x[s], lam, ga, gd);
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (r < nst) {
            row[r * 2 * S + s] = ga[r] * as[r] * (1.f - as[r]);
            row[r * 2 * S + S + s] = gd[r] * ds[r] * (1.f - ds[r]);
          }
      }
    }
  }
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(RF_NT) refine_kernel(const RfK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  constexpr int RW = FWD_ROW(SM);
  extern __shared__ __attribute__((aligned(16))) float s_rf[];
  const FwdK& f = k.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, Q = f.Q, H = f.H, nd = k.d.nd, nj = k.nj, B = f.B;
  const int nst = fixed_step_evals(f.method, f.R);   // stages of one step: euler 1, midpoint 2, rk4 4 (the last one the next step's first)
  const int nch = RF_NT / H, nsamp = (T - 1) * nst;
  const FwdSm sm = fwd_sm(s_rf, k.o.f);
  const ScoredSm ss = scored_sm(s_rf, k.o.s);
  float* s_ak = s_rf + k.o.ak;       // [T-1][S] the step coefficients A of the draw (the scan overwrites sm.A with the states)
  float* s_g = s_rf + k.o.g;         // [T][S] g_x, then lambda
  float* s_tab = s_rf + k.o.tab;     // [(T-1) nst][2 S] g_pre_a | g_pre_d
  float* s_part = s_rf + k.o.part;   // [H][nch] per-chunk partials of g_u
  float* s_gu = s_rf + k.o.gu;       // [2 H] g_u | the init net's hidden gradient
  float* s_loss = s_rf + k.o.loss;   // [K] the per-draw losses of the iteration
  float* s_fj = s_rf + k.o.fj;       // [1] F_j

  // ---- R0 ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  tb_stage_scales(k.d, ss, C * T, tid);

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    // ---- R1 ----
    __syncthreads();   // (R0's writes; the previous trajectory's readers of every table are done)
    if (tid < k.pr.nu) sm.u[tid] = slode_label_at(k.d.lab, k.d.u, k.pr.nu, b, tid);
    tb_stage_obs<true>(k.d, ss, b, T, C, tid);
    __syncthreads();
    // thread l < L keeps its latent dim: phi = (loc, rho), the prior, Adam's moments, the best iterate
    TbDim q;   // (loc, sc: the iterate; nlsc = -rho)
    // (the optimiser's own arithmetic -- two parameters per thread, once per iteration -- runs in fp64 on fp64 master copies of phi: in fp32
    // the constants 0.001f and 1 - 0.999f alone disagree by 1.3e-5, a 7e-6 error of every step length, and the iterates drift from the
    // exact loop's by 5e-7 per step; the forward and backward passes take phi rounded to fp32)
    double loc_d = 0.0, rho_d = 0.0, m_l = 0.0, v_l = 0.0, m_r = 0.0, v_r = 0.0, b1t = 1.0, b2t = 1.0;
    float best_loc = 0.f, best_sc = 1.f, best_f = 0.f, f0 = 0.f;
    int best_j = 0;
    if (tid < L) {
      tb_dim_load(q, k.d, k.pr, f.params, sm.u, b, L, tid, true);
      loc_d = (double)q.loc; rho_d = (double)-q.nlsc;
    }
    for (int j = 0; j <= nj; ++j) {
      const bool bwd = j < nj || (j == 0 && k.grad0_out != nullptr);   // (workgroup-uniform)
      float g_loc = 0.f, g_rho = 0.f;
      for (int kk = 0; kk < nd; ++kk) {
        // ---- R2 ----
        float klt = 0.f, z = 0.f, eps = 0.f;
        if (tid < L) {
          eps = slode_eps_at(k.d.rng, k.d.eps, b, L, tid, kk, B);
          z = fmaf(q.sc, eps, q.loc);
          klt = tb_logq_minus_logp(z, q.loc, q.sc, q.nlsc, q.pl, q.pls, q.ips);
          sm.z[tid] = z;
        }
        __syncthreads();   // (also: the previous draw's readers of every table of the draw are done)
        // ---- R3 ----
        fwd_init_state<SM>(sm, H, L, S, tid);
        fwd_step_table_staged<SM>(f, sm, S, 0, T - 1, tid);
        __syncthreads();
        if (bwd) {
          for (int i = tid; i < (T - 1) * S; i += RF_NT) s_ak[i] = sm.A[i];
          __syncthreads();
        }
        fwd_scan(sm.A, sm.B, sm.x0, S, T - 1, lane, wave, RF_NT / 64);
        __syncthreads();
        // ---- R4 ----
        const float llt0 = tb_loglik_weighted<SM, true>(sm, S, T, C, Q, k.d.gauss, k.d.tau, ss, bwd, s_g, tid);
        // ---- R5 (its barrier also publishes R4's g_x) ----
        tb_draw_sums(klt, llt0, ss.red, nullptr, 0, s_loss + kk, nullptr);
        if (bwd) {
          // ---- R6 ----
          rf_rev_scan(s_g, s_ak, S, T - 1, lane, wave, RF_NT / 64);
          __syncthreads();
          // ---- R7 ----
          rf_step_table_bwd<SM>(f, sm, S, nst, s_g, s_tab, tid);
          __syncthreads();
          // ---- R8 ----
          if (tid < H * nch) {
            const int jh = tid / nch, ch = tid - jh * nch;
            float r[RW];
#pragma unroll
            for (int i = 0; i < RW; ++i) r[i] = sm.row[jh * RW + i];
            float acc = 0.f;
            for (int i = ch; i < nsamp; i += nch) {
              const int n = i / nst, rr = i - n * nst;
              const float t = f.stage_t[(long long)n * f.R + rr];
              const float* tb = s_tab + (long long)i * 2 * S;
              float v = 0.f;
#pragma unroll
              for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(tb[S + s], r[2 + SM + s], fmaf(tb[s], r[2 + s], v));
              if (fmaf(r[0], t, r[1]) > 0.f) acc += v;
            }
            s_part[tid] = acc;
          }
          __syncthreads();
          // ---- R9 ----
          if (tid < H) {
            float gu = 0.f;
            for (int c = 0; c < nch; ++c) gu += s_part[tid * nch + c];
            s_gu[tid] = gu;
          } else if (tid < 2 * H) {
            const int jh = tid - H;
            float gh = 0.f;
            for (int s = 0; s < S; ++s) { const float x0 = sm.x0[s]; gh = fmaf(sm.w2[jh * S + s], s_g[s] * x0 * (1.f - x0), gh); }
            s_gu[tid] = sm.h0[jh] > 0.f ? gh : 0.f;
          }
          __syncthreads();
          // ---- R10 ----
          if (tid < L) {
            float gz = 0.f;
            for (int r = 0; r < 2 * H; ++r) gz = fmaf(sm.w1[tid * 2 * H + r], s_gu[r], gz);
            gz += (z - q.pl) * q.ips * q.ips;
            g_loc += gz;
            g_rho += gz * q.sc * eps - 1.f;
          }
        }
      }
      // ---- F_j, the best iterate, Adam ----
      __syncthreads();   // (the draws' losses)
      if (tid == 0) {
        double sl = 0.0;
        for (int q = 0; q < nd; ++q) sl += (double)s_loss[q];
        const float fj = (float)(sl / (double)nd);
        s_fj[0] = fj;
        if (k.trace_out) k.trace_out[(long long)j * B + b] = fj;
      }
      __syncthreads();
      const float fj = s_fj[0];
      if (j == 0) f0 = fj;
      if (j == 0 || fj < best_f) { best_f = fj; best_loc = q.loc; best_sc = q.sc; best_j = j; }
      if (tid < L) {
        const float inv_k = 1.f / (float)nd;
        g_loc *= inv_k; g_rho *= inv_k;
        if (j == 0 && k.grad0_out) { k.grad0_out[(long long)b * 2 * L + tid] = g_loc; k.grad0_out[(long long)b * 2 * L + L + tid] = g_rho; }
        if (j < nj) {   // Adam, beta = (0.9, 0.999), eps 1e-8, bias correction
          const double gl = (double)g_loc, gr = (double)g_rho, lr = (double)k.lr;
          b1t *= 0.9; b2t *= 0.999;
          m_l = 0.9 * m_l + (1.0 - 0.9) * gl; v_l = 0.999 * v_l + (1.0 - 0.999) * gl * gl;
          m_r = 0.9 * m_r + (1.0 - 0.9) * gr; v_r = 0.999 * v_r + (1.0 - 0.999) * gr * gr;
          const double c1 = 1.0 - b1t, c2 = 1.0 - b2t;
          loc_d -= lr * (m_l / c1) / (sqrt(v_l / c2) + 1e-8);
          rho_d -= lr * (m_r / c1) / (sqrt(v_r / c2) + 1e-8);
          q.loc = (float)loc_d; q.nlsc = -(float)rho_d;
          q.sc = expf(-q.nlsc);
        }
      }
    }
    if (tid < L) { k.loc_out[(long long)b * L + tid] = best_loc; k.scale_out[(long long)b * L + tid] = best_sc; }
    if (tid == 0) {
      k.elbo_out[(long long)b * 2] = f0; k.elbo_out[(long long)b * 2 + 1] = best_f;
      if (k.best_step) k.best_step[b] = best_j;
    }
  }
}

RfLds rf_lds(const slode_shape& s, int nd, bool generic) {
  const int nst = fixed_step_evals(s.method), cap = SLODE_REFINE_LDS_MAX / 4;
  LdsCarve cv;
  RfLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.s = scored_lds(cv, s, true, 0, 0);
  o.ak = cv.take((s.T - 1) * s.S); o.g = cv.take(s.T * s.S); o.tab = cv.take((s.T - 1) * nst * 2 * s.S);
  o.part = cv.take(RF_NT); o.gu = cv.take(2 * s.H);
  // the K losses come last; a K that cannot fit anyway counts as the whole budget (no overflow of the offsets)
  o.loss = cv.take(nd < cap ? (nd < 0 ? 0 : nd) : cap); o.fj = cv.take(4);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_refine_lds_bytes(const slode_shape& s, int num_draws, int force_generic) {
  return (size_t)rf_lds(s, num_draws, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_refine(const RefineLaunch& a, hipStream_t stream) {
  const ScoredLaunch& d = a.d;
  const slode_shape& s = d.s;
  RfK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay); fwd_fill(k.d, d);
  k.nj = a.num_steps; k.lr = a.lr;
  k.loc_out = a.loc_out; k.scale_out = a.scale_out; k.elbo_out = a.elbo_out; k.grad0_out = a.grad0_out; k.trace_out = a.trace_out;
  k.best_step = a.best_step;
  k.o = rf_lds(s, d.num_draws, fwd_generic(s, d.force_generic));
  const size_t lds = slode_refine_lds_bytes(s, d.num_draws, d.force_generic);
  // the kernel's thread maps: 2 H threads for the two hidden layers, H x (256 / H) for the hidden-unit sums, L threads for the latent dims
  if (lds > SLODE_REFINE_LDS_MAX || d.num_draws < 1 || a.num_steps < 0 || d.grid < 1 || s.T < 2 || s.H < 1 || 2 * s.H > RF_NT || s.L > RF_NT ||
      (s.aux_in_main && s.n_aux > 0))
    return hipErrorInvalidValue;
  fwd_dispatch(s, d.force_generic, [&](auto sc) {
    constexpr int SC = decltype(sc)::value;
    fwd_launch("posterior_refine", refine_kernel<SC>, d.grid, lds, stream, k);
  });
  return hipGetLastError();
}
