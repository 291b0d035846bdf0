// Counterfactual curves (slode_intervene_moments): per trajectory, over num_samples PAIRED latent draws, the mean and the population standard
// deviation of every decoder head curve under swapped labels (v_cf) and of its difference to the subject's own curve (v_cf - v_f) -- without
// writing anything sized num_samples x B x C x T.  Both arms of a draw share ONE noise row:
//   factual         z_f  = loc_q(x_b) + scale_q(x_b) * eps                       (the posterior draw of recon_moments_kernel, is_post)
//   counterfactual  z_cf = z_f outside every intervened prior group; inside group g: ploc_g(u'_b) + exp(pls_g(u'_b)) * eps
// The phases are those of the draw loop of slode_forward.h; M1 and M2 are this kernel's own (both distributions at once),
// M3-M6 run once per arm.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in order:
//   M0  once per workgroup: fwd_stage_weights -- both arms of every draw of every trajectory reuse them
//   M1  once per trajectory: the counterfactual labels of the intervened groups; per latent dim the posterior loc / scale (from the encoder
//       launch) and the counterfactual loc / scale (the group's conditional prior nets on u' inside an intervened group, else the posterior's)
//   per draw: one noise value per latent dim (row k * B + b of ONE drawing call, or of the explicit [ns, B, L] tensor), kept by its thread
//   per arm (factual, then counterfactual):
//   M2  z = loc + scale * eps_k with the arm's loc / scale
//   M3-M5  fwd_solve over the whole grid
//   M6  thread <-> time point: the Q * C head values v.  Factual arm: kept in the LDS ([Q*C][T], the thread's own slots).  Counterfactual arm:
//       two sets of running moments of (q, c, t) (fwd_moment_add): of v_cf and of e = v_cf - v_f
//   M7  once per trajectory: fwd_moment_store of both sets, written with T contiguous
// The moments (and the kept factual values) of (q, c, t) belong to ONE thread for the whole trajectory, which takes the draws in the fixed
// order k = 0 .. ns - 1: the result is a function of (parameters, inputs, labels, noise) alone -- independent of the grid, bitwise
// reproducible, no atomics.  With no group intervened both arms run the same operations on the same z: the effect is exactly 0.
#include "slode_forward.h"

namespace {

constexpr int IV_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct IvLds { FwdLds f; int acc, vf; LocScLds post, cf; int total; };

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
  const int tid = threadIdx.x;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.ns;
  const FwdSm sm = fwd_sm(s_iv, k.o.f);   // (sm.u: u', only the columns of intervened groups are filled and read)
  float* s_acc = s_iv + k.o.acc;   // [Q*C][6: v0, s1, s2 of v_cf | v0, s1, s2 of v_cf - v_f][T]
  float* s_vf = s_iv + k.o.vf;     // [Q*C][T]: the factual head values of the current draw
  float* s_loc = s_iv + k.o.post.loc;   // posterior loc / scale
  float* s_sc = s_iv + k.o.post.sc;
  float* s_cloc = s_iv + k.o.cf.loc;    // counterfactual loc / scale
  float* s_csc = s_iv + k.o.cf.sc;
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
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
        // ---- M6: head values of the thread's time points; factual: kept; counterfactual: both running moment sets ----
        for (int t = tid; t < T; t += IV_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, t, x);
          for (int qc = 0; qc < QC; ++qc) {
            const float v = fwd_head_value<SM>(sm, S, qc, x);
            if (arm == 0) {
              s_vf[qc * T + t] = v;
            } else {
              float* m = s_acc + (qc * 6) * T + t;
              fwd_moment_add(m, T, kk == 0, v);
              if (need_f) fwd_moment_add(m + 3 * T, T, kk == 0, v - s_vf[qc * T + t]);
            }
          }
        }
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    const float inv = 1.0f / (float)ns;
    for (int t = tid; t < T; t += IV_NT)
      for (int qc = 0; qc < QC; ++qc) {
        const int q = qc / C, c = qc - q * C;
        const float* m = s_acc + (qc * 6) * T + t;
        const long long o = (((long long)q * f.B + b) * C + c) * T + t;
        fwd_moment_store(m, T, inv, k.cf_mean, k.cf_sd, o);
        if (need_f) fwd_moment_store(m + 3 * T, T, inv, k.eff_mean, k.eff_sd, o);
      }
  }
}

IvLds iv_lds(const slode_shape& s, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  IvLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 6 * s.T); o.vf = cv.take(Q * s.C * s.T);
  o.post = fwd_lds_loc_sc(cv, s); o.cf = fwd_lds_loc_sc(cv, s);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_intervene_moments_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)iv_lds(s, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_intervene_moments(const InterveneMomentsLaunch& a, hipStream_t stream) {
  const DrawsLaunch& d = a.d;
  const slode_shape& s = d.s;
  IvK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay);
  k.ns = d.num_samples; k.mask = (int)a.group_mask;
  k.loc = d.loc; k.scale = d.scale; k.eps = d.eps;
  k.cf_mean = a.cf_mean; k.cf_sd = a.cf_sd; k.eff_mean = a.eff_mean; k.eff_sd = a.eff_sd;
  k.rng = d.rng; k.cf = a.cf; k.o = iv_lds(s, fwd_generic(s, d.force_generic));
  const size_t lds = slode_intervene_moments_lds_bytes(s, d.force_generic);
  if (lds > SLODE_INTERVENE_MOMENTS_LDS_MAX || d.num_samples < 1 || d.grid < 1 || (a.group_mask != 0 && a.cf.n < 1)) return hipErrorInvalidValue;
  fwd_dispatch(s, d.force_generic, [&](auto sc) { fwd_launch("intervene_moments", intervene_moments_kernel<decltype(sc)::value>, d.grid, lds, stream, k); });
  return hipGetLastError();
}
