// Counterfactual curves (slode_intervene_moments): per trajectory, over num_samples PAIRED latent draws, the mean and the population standard
// deviation of every decoder head curve under swapped labels (v_cf) and of its difference to the subject's own curve (v_cf - v_f) -- without
// writing anything sized num_samples x B x C x T.  Both arms of a draw share ONE noise row:
//   factual         z_f  = loc_q(x_b) + scale_q(x_b) * eps                       (the posterior draw of recon_moments_kernel, is_post)
//   counterfactual  z_cf = z_f outside every intervened prior group; inside group g: ploc_g(u'_b) + exp(pls_g(u'_b)) * eps
// The phases are those of recon_moments_kernel.hip (M0-M7), the forward ones (M0, M3-M5, the prior nets of M1) shared through
// slode_forward.h; M3-M6 run once per arm.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in order:
//   M0  once per workgroup: [w_t | u_j | W_g | W_d] per hidden unit, the z-columns of the hidden layer and the init net (transposed), the
//       init net's output layer, the head weights and the biases into the LDS -- both arms of every draw of every trajectory reuse them
//   M1  once per trajectory: the counterfactual labels of the intervened groups; per latent dim the posterior loc / scale (from the encoder
//       launch) and the counterfactual loc / scale (the group's conditional prior nets on u' inside an intervened group, else the posterior's)
//   per draw: one noise value per latent dim (row k * B + b of ONE drawing call, or of the explicit [ns, B, L] tensor), kept by its thread
//   per arm (factual, then counterfactual):
//   M2  z = loc + scale * eps_k with the arm's loc / scale
//   M3  time-invariant part of the hidden layer (into the unit's weight row) and the init net; x0
//   M4  step coefficients x' = A x + b of every grid step (tests/kernel_math.py step_coeffs), thread <-> step, weights from the LDS
//   M5  forward affine scan (one solve on all four waves): one state component per wave pass
//   M6  thread <-> time point: the Q * C head values v.  Factual arm: kept in the LDS ([Q*C][T], the thread's own slots).  Counterfactual arm:
//       two sets of running moments of (q, c, t), each shifted by its first draw's value: of v_cf and of e = v_cf - v_f
//       (s1 += v - v0, s2 += (v - v0)^2 -- no sum of squares of the values themselves)
//   M7  once per trajectory: mean = v0 + s1 / ns, sd = sqrt(max(0, s2 - s1^2 / ns) / ns) of both sets, written with T contiguous
// The moments (and the kept factual values) of (q, c, t) belong to ONE thread for the whole trajectory, which takes the draws in the fixed
// order k = 0 .. ns - 1: the result is a function of (parameters, inputs, labels, noise) alone -- independent of the grid, bitwise
// reproducible, no atomics.  With no group intervened both arms run the same operations on the same z: the effect is exactly 0.
#include "slode_forward.h"

namespace {

constexpr int IV_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct IvLds { FwdLds f; int acc, vf, loc, sc, cloc, csc, total; };

struct IvK {
  FwdK f;
  PriorK pr;
  int ns, mask;
  const float *loc, *scale, *eps;
  float *cf_mean, *cf_sd, *eff_mean, *eff_sd;
  IvLds o;
  RngK rng;
  LabelSrc cf;   // the counterfactual label tensors, one by one (n >= 1 whenever mask != 0)
};

// one running moment set [v0 | s1 | s2] (T floats apart) of the thread's (q, c, t), draw kk
__device__ __forceinline__ void iv_moment(float* m, int T, int kk, float v) {
  if (kk == 0) { m[0] = v; m[T] = 0.f; m[2 * T] = 0.f; }
  else { const float dv = v - m[0]; m[T] += dv; m[2 * T] = fmaf(dv, dv, m[2 * T]); }
}

// column `col` of u' from the counterfactual label tensors (slode_label_at without the one-dense-matrix form, which this call does not take)
__device__ __forceinline__ float iv_label_at(const LabelSrc& ls, long long b, int col) {
  int i = 0;
#pragma unroll
  for (int q = 1; q < SLODE_MAX_LABELS; ++q) i = (q < ls.n && col >= ls.off[q]) ? q : i;
  const int w = ls.off[i + 1] - ls.off[i];
  return ls.p[i][b * w + (col - ls.off[i])];
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(IV_NT) intervene_moments_kernel(const IvK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_iv[];
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, H = f.H, C = f.C, NS = T - 1, QC = f.Q * C, ns = k.ns;
  const FwdSm sm = fwd_sm(s_iv, k.o.f);   // (sm.u: u', only the columns of intervened groups are filled and read)
  float* s_acc = s_iv + k.o.acc;   // [Q*C][6: v0, s1, s2 of v_cf | v0, s1, s2 of v_cf - v_f][T]
  float* s_vf = s_iv + k.o.vf;     // [Q*C][T]: the factual head values of the current draw
  float* s_loc = s_iv + k.o.loc;   // posterior loc / scale
  float* s_sc = s_iv + k.o.sc;
  float* s_cloc = s_iv + k.o.cloc; // counterfactual loc / scale
  float* s_csc = s_iv + k.o.csc;
  const bool need_f = k.eff_mean || k.eff_sd;   // (workgroup-uniform: the factual arm serves the effect alone)

  // ---- M0: the weights every solve reuses ----
  fwd_stage_weights<SM>(f, sm, S, tid);

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- M1 ----
    __syncthreads();   // (M0's writes; the previous trajectory's readers of s_u / s_loc / s_sc / s_cloc / s_csc)
    if (tid < k.pr.nu) {
      int hit = 0;
      for (int g = 0; g < k.pr.n_groups; ++g)
        if (((k.mask >> g) & 1) && tid >= k.pr.grp[g].u_off && tid < k.pr.grp[g].u_off + k.pr.grp[g].u_dim) hit = 1;
      if (hit) sm.u[tid] = iv_label_at(k.cf, b, tid);
    }
    __syncthreads();
    if (tid < L) {
      const int l = tid;
      const float loc = k.loc[(long long)b * L + l], sc = k.scale[(long long)b * L + l];
      float cloc = loc, csc = sc, pl, pls;
      if (fwd_prior_at(k.pr, par, sm.u, l, pl, pls, k.mask)) { cloc = pl; csc = expf(pls); }
      s_loc[l] = loc; s_sc[l] = sc; s_cloc[l] = cloc; s_csc[l] = csc;   // (read back by this thread alone)
    }
    for (int kk = 0; kk < ns; ++kk) {
      // draw kk = row kk * B + b of the call's noise: ONE value per latent dim, shared by both arms
      const float e = tid < L ? slode_eps_at(k.rng, k.eps, (long long)kk * f.B + b, L, tid) : 0.f;
      for (int arm = need_f ? 0 : 1; arm < 2; ++arm) {
        // ---- M2 ----
        if (tid < L) sm.z[tid] = arm ? fmaf(s_csc[tid], e, s_cloc[tid]) : fmaf(s_sc[tid], e, s_loc[tid]);
        __syncthreads();   // (also: the previous solve's readers of s_A / s_x0 / s_row[.][1] are done)
        // ---- M3: u = W_z z + b_h into the units' rows; the init net's hidden layer ----
        fwd_init_state<SM>(sm, H, L, S, tid);
        // ---- M4: step coefficients ----
        fwd_step_table_staged<SM>(f, sm, S, tid);
        __syncthreads();
        // ---- M5: forward affine scan, in place: x[n + 1][s] takes the slot of A[n][s] ----
        fwd_scan(sm.A, sm.B, sm.x0, S, NS, lane, wave, IV_NT / 64);
        __syncthreads();
        // ---- M6: head values of the thread's time points; factual: kept; counterfactual: both running moment sets ----
        for (int t = tid; t < T; t += IV_NT) {
          float x[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) x[s] = s < S ? (t == 0 ? sm.x0[s] : sm.A[(t - 1) * S + s]) : 0.f;
          for (int qc = 0; qc < QC; ++qc) {
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(sm.hw[qc * S + s], x[s], v);
            if (arm == 0) {
              s_vf[qc * T + t] = v;
            } else {
              float* m = s_acc + (qc * 6) * T + t;
              iv_moment(m, T, kk, v);
              if (need_f) iv_moment(m + 3 * T, T, kk, v - s_vf[qc * T + t]);
            }
          }
        }
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    {
      const float inv = 1.0f / (float)ns;
      for (int t = tid; t < T; t += IV_NT)
        for (int qc = 0; qc < QC; ++qc) {
          const int q = qc / C, c = qc - q * C;
          const float* m = s_acc + (qc * 6) * T + t;
          const long long o = (((long long)q * f.B + b) * C + c) * T + t;
          {
            const float s1 = m[T], s2 = m[2 * T];
            if (k.cf_mean) k.cf_mean[o] = fmaf(s1, inv, m[0]);
            if (k.cf_sd) k.cf_sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
          }
          if (need_f) {
            const float s1 = m[4 * T], s2 = m[5 * T];
            if (k.eff_mean) k.eff_mean[o] = fmaf(s1, inv, m[3 * T]);
            if (k.eff_sd) k.eff_sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
          }
        }
    }
  }
}

IvLds iv_lds(const slode_shape& s, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  IvLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 6 * s.T); o.vf = cv.take(Q * s.C * s.T);
  o.loc = cv.take(s.L); o.sc = cv.take(s.L); o.cloc = cv.take(s.L); o.csc = cv.take(s.L);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_intervene_moments_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)iv_lds(s, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_intervene_moments(const InterveneMomentsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  IvK k{};
  fwd_fill(k.f, s, lay, a.params, a.times, a.stage_t); fwd_fill(k.pr, s, lay);
  k.ns = a.num_samples; k.mask = (int)a.group_mask;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps;
  k.cf_mean = a.cf_mean; k.cf_sd = a.cf_sd; k.eff_mean = a.eff_mean; k.eff_sd = a.eff_sd;
  k.rng = a.rng; k.cf = a.cf; k.o = iv_lds(s, fwd_generic(s, a.force_generic));
  const size_t lds = slode_intervene_moments_lds_bytes(s, a.force_generic);
  if (lds > SLODE_INTERVENE_MOMENTS_LDS_MAX || a.num_samples < 1 || a.grid < 1 || (a.group_mask != 0 && a.cf.n < 1)) return hipErrorInvalidValue;
  fwd_dispatch(s, a.force_generic, [&](auto sc) { fwd_launch("intervene_moments", intervene_moments_kernel<decltype(sc)::value>, a.grid, lds, stream, k); });
  return hipGetLastError();
}
