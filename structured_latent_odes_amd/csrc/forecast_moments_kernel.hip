// Forecast moments (slode_forecast_moments): per trajectory, the mean and the population standard deviation over num_samples latent draws
// of every decoder head curve -- and, when asked, of the ODE state -- on an output grid times_out[0 .. T_out) that is the call's own
// argument: longer, shorter or finer than the training grid of the shape.  The draws are those of slode_recon_moments; only the solve and
// the heads run on the other grid.  The grid is walked in WINDOWS of W steps, so the LDS tables are sized by W and not by T_out.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid).  Windows outer, draws inner:
//   M0  once per workgroup: the staged weights of slode_forward.h
//   M1  once per trajectory: labels; loc / scale of the posterior (from the encoder launch) or of the conditional prior nets
//   per window w -- steps [w W, min((w + 1) W, T_out - 1)), time points w W + 1 .., point 0 added to window 0 -- and per draw k = 0 .. ns - 1:
//   M2  z = loc + scale * eps_k again, from the same Philox counter or the same eps row: nothing per draw is kept but the carry
//   M3  fwd_init_state: the window-invariant part (the units' rows of this z; x0) -- the same operations every time
//   M4  step coefficients of the window's steps only, times_out / stage_t_out read at the window's offset
//   M5  fwd_scan over the window's steps from x0 (window 0) or from the draw's carry; then the state at the window's last point -> carry[k]
//   M6  thread <-> time point of the window: head values (and the states) with shifted running moments, v0, s1 += v - v0, s2 += (v - v0)^2
//   M7  after the window's last draw: mean = v0 + s1 / ns, sd = sqrt(max(0, s2 - s1^2 / ns) / ns) of the window's points, T_out contiguous
// Every (q, c, t) and (s, t) has ONE owner thread, which sees the draws in the order k = 0 .. ns - 1: no atomics, no merge; the result is a
// function of (parameters, inputs, noise, output grid, W) alone, bitwise reproducible and independent of the launch grid.  W decides which
// scan chunk a step falls into, i.e. how the affine maps are associated: two windows agree to fp32 rounding, not bitwise.
// (This kernel keeps its own text of M1, M2, M6, M7 and of the M3-M5 sequence: written through the draw-loop routines of slode_forward.h it
// measured 2-3 % slower wherever a t loop takes more than one thread round -- DESIGN 3.13.  The step table is the shared one.)
#include "slode_forward.h"

namespace {

constexpr int FC_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones (A | b sized for W steps), then the moments
// of the heads and of the states over the W + 1 points of a window, loc | scale and the carry table
struct FcLds { FwdLds f; int acc, xacc, loc, sc, carry, total; };

struct FcK {
  FwdK f;   // (T, times, stage_t: the OUTPUT grid)
  PriorK pr;
  int is_post, ns, W, states;
  const float *loc, *scale, *eps, *u;
  float *mean, *sd, *x_mean, *x_sd;
  FcLds o;
  RngK rng;
  LabelSrc lab;
};

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(FC_NT) forecast_moments_kernel(const FcK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_fc[];
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, H = f.H, C = f.C, NS = T - 1, QC = f.Q * C, ns = k.ns, W = k.W, P = W + 1;
  const FwdSm sm = fwd_sm(s_fc, k.o.f);
  float* s_acc = s_fc + k.o.acc;      // [Q*C][3: v0, s1, s2][W + 1]
  float* s_xacc = s_fc + k.o.xacc;    // [S][3][W + 1] (states asked)
  float* s_loc = s_fc + k.o.loc;
  float* s_sc = s_fc + k.o.sc;
  float* s_carry = s_fc + k.o.carry;  // [ns][S]: the state of draw k at the last point of the previous window

  // ---- M0: the weights every draw reuses ----
  fwd_stage_weights<SM>(f, sm, S, tid);

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- M1 ----
    __syncthreads();   // (M0's writes; the previous trajectory's readers of s_u / s_loc / s_sc)
    if (!k.is_post && k.pr.n_groups > 0 && tid < k.pr.nu) sm.u[tid] = slode_label_at(k.lab, k.u, k.pr.nu, b, tid);   // (only the conditional prior nets read labels)
    __syncthreads();
    if (tid < L) {
      const int l = tid;
      float loc, sc;
      if (k.is_post) {
        loc = k.loc[(long long)b * L + l]; sc = k.scale[(long long)b * L + l];
      } else {
        float pl, pls;
        fwd_prior_at(k.pr, par, sm.u, l, pl, pls);
        loc = pl; sc = expf(pls);
      }
      s_loc[l] = loc; s_sc[l] = sc;
    }
    for (int n_lo = 0; n_lo < NS; n_lo += W) {
      const int n_hi = min(n_lo + W, NS), nw = n_hi - n_lo;
      const int j_lo = n_lo == 0 ? 0 : 1;   // the window's points: slots j_lo .. nw, slot j = time point n_lo + j (slot 0: x0, window 0 alone)
      for (int kk = 0; kk < ns; ++kk) {
        // ---- M2: draw kk = row kk * B + b of the call's noise ----
        if (tid < L) sm.z[tid] = fmaf(s_sc[tid], slode_eps_at(k.rng, k.eps, (long long)kk * f.B + b, L, tid), s_loc[tid]);
        __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
        // ---- M3: u = W_z z + b_h into the units' rows; the init net's hidden layer; x0 ----
        fwd_init_state<SM>(sm, H, L, S, tid);
        // ---- M4: step coefficients of the window's steps ----
        fwd_step_table_staged<SM>(f, sm, S, n_lo, n_hi, tid);
        __syncthreads();
        // ---- M5: forward affine scan of the window, in place: x[n_lo + i + 1][s] takes the slot of A[i][s] ----
        fwd_scan(sm.A, sm.B, n_lo == 0 ? sm.x0 : s_carry + kk * S, S, nw, lane, wave, FC_NT / 64);
        __syncthreads();
        if (tid < S) s_carry[kk * S + tid] = sm.A[(nw - 1) * S + tid];   // (its next reader: this draw's scan of the next window)
        // ---- M6: head values (and states) of the thread's time points, running moments ----
        for (int j = j_lo + tid; j <= nw; j += FC_NT) {
          float x[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) x[s] = s < S ? (j == 0 ? sm.x0[s] : sm.A[(j - 1) * S + s]) : 0.f;
          for (int qc = 0; qc < QC; ++qc) {
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(sm.hw[qc * S + s], x[s], v);
            float* m = s_acc + (qc * 3) * P + j;
            if (kk == 0) { m[0] = v; m[P] = 0.f; m[2 * P] = 0.f; }
            else { const float dv = v - m[0]; m[P] += dv; m[2 * P] = fmaf(dv, dv, m[2 * P]); }
          }
          if (k.states) {
#pragma unroll
            for (int s = 0; s < SM; ++s)
              if (s < S) {
                float* m = s_xacc + (s * 3) * P + j;
                if (kk == 0) { m[0] = x[s]; m[P] = 0.f; m[2 * P] = 0.f; }
                else { const float dv = x[s] - m[0]; m[P] += dv; m[2 * P] = fmaf(dv, dv, m[2 * P]); }
              }
          }
        }
      }
      // ---- M7: the thread's own (q, c, t) and (s, t) of this window: no barrier needed; lanes <-> consecutive t: coalesced stores ----
      {
        const float inv = 1.0f / (float)ns;
        for (int j = j_lo + tid; j <= nw; j += FC_NT) {
          const long long t = (long long)n_lo + j;
          for (int qc = 0; qc < QC; ++qc) {
            const int q = qc / C, c = qc - q * C;
            const float* m = s_acc + (qc * 3) * P + j;
            const float s1 = m[P], s2 = m[2 * P];
            const long long o = (((long long)q * f.B + b) * C + c) * T + t;
            k.mean[o] = fmaf(s1, inv, m[0]);
            if (k.sd) k.sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
          }
          if (k.states)
            for (int s = 0; s < S; ++s) {
              const float* m = s_xacc + (s * 3) * P + j;
              const float s1 = m[P], s2 = m[2 * P];
              const long long o = ((long long)b * S + s) * T + t;
              if (k.x_mean) k.x_mean[o] = fmaf(s1, inv, m[0]);
              if (k.x_sd) k.x_sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
            }
        }
      }
    }
  }
}

// the pieces for a window of W steps: fwd_lds on a shape whose T is the window's point count gives A | b of W S floats each
FcLds fc_lds(const slode_shape& s, int ns, int states, int W, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  slode_shape sw = s;
  sw.T = W + 1;
  LdsCarve cv;
  FcLds o{};
  o.f = fwd_lds(cv, sw, generic);
  o.acc = cv.take(Q * s.C * 3 * (W + 1)); o.xacc = cv.take(states ? s.S * 3 * (W + 1) : 0);
  o.loc = cv.take(s.L); o.sc = cv.take(s.L); o.carry = cv.take(ns * s.S);
  o.total = cv.n;
  return o;
}

}  // namespace

// W <= SLODE_FORECAST_MAX_T and ns < 2^30 / S keep every piece inside an int (the callers' ranges; the result is compared with the budget)
size_t slode_forecast_lds_bytes(const slode_shape& s, int num_samples, int want_states, int window, int force_generic) {
  if ((long long)num_samples * s.S > (1 << 28)) return (size_t)1 << 32;   // (a carry table far beyond any budget: no int overflow below)
  return (size_t)fc_lds(s, num_samples, want_states, window, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_forecast_moments(const ForecastMomentsLaunch& a, hipStream_t stream) {
  const DrawsLaunch& d = a.d;
  const slode_shape& s = d.s;
  if (d.num_samples < 1 || d.grid < 1 || a.T_out < 2 || a.window < 1 || a.window > a.T_out - 1 || !a.mean) return hipErrorInvalidValue;
  const int states = (a.x_mean || a.x_sd) ? 1 : 0;
  const size_t lds = slode_forecast_lds_bytes(s, d.num_samples, states, a.window, d.force_generic);
  if (lds > SLODE_FORECAST_LDS_MAX) return hipErrorInvalidValue;
  FcK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay);
  k.f.T = a.T_out;
  k.is_post = d.is_post; k.ns = d.num_samples; k.W = a.window; k.states = states;
  k.loc = d.loc; k.scale = d.scale; k.eps = d.eps; k.u = d.u;
  k.mean = a.mean; k.sd = a.sd; k.x_mean = a.x_mean; k.x_sd = a.x_sd; k.rng = d.rng; k.lab = d.lab;
  k.o = fc_lds(s, d.num_samples, states, a.window, fwd_generic(s, d.force_generic));
  fwd_dispatch(s, d.force_generic, [&](auto sc) { fwd_launch("forecast_moments", forecast_moments_kernel<decltype(sc)::value>, d.grid, lds, stream, k); });
  return hipGetLastError();
}
