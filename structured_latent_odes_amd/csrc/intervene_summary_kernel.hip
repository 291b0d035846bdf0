// Counterfactual summaries (slode_intervene_summary): per trajectory, head curve and channel, over num_samples PAIRED latent draws, the mean and
// the population standard deviation of the eight curve functionals of slode_curve_summary -- peak, time of peak, trough, time of trough,
// trapezoid area, time beyond a threshold, first time beyond it, whether it is crossed at all -- of the subject's own curve (factual), of its
// curve under each of V hypothesised inputs (cf) and of the paired difference cf - factual (effect).  Nothing sized num_samples x B x C x T is
// written, and the encoder and the factual arm run once for all V hypotheses.  All V + 1 arms of a draw share ONE noise row:
//   factual  z_f    = loc_q(x_b) + scale_q(x_b) * eps                       (the posterior draw of curve_summary_kernel, is_post)
//   arm v    z_cf,v = z_f outside every intervened prior group; inside group g: ploc_g(u'_{b,v}) + exp(pls_g(u'_{b,v})) * eps
//   u'_{b,v}: row b's own label row with the columns of every hypothesised label tensor replaced by row v of its table (label_evidence's rule)
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in that
// order.  The frame is the draw loop of slode_forward.h; M1 and M2 are intervene_moments_kernel's (fwd_prior_at on u' with the
// group mask: an arm's latent has that kernel's bits), M6 is curve_summary_kernel's:
//   M0  once per workgroup: fwd_stage_weights; the grid t[T] and the trapezoid node weights w[T] in fp32
//   M1  once per trajectory: the posterior loc | scale; per arm v the labels u'_{b,v} of the intervened groups and the counterfactual
//       loc | scale into [V][2 L] of the LDS (outside the intervened groups: the posterior's)
//   per draw: one noise value per latent dim, kept in a register by its thread across all arms
//   per arm (factual first, then v = 0 .. V - 1):
//   M2  z = loc + scale * eps with the arm's loc / scale
//   M3-M5  fwd_solve over the whole grid
//   M6a thread <-> time point: the Q * C head values into the table val[Q*C][T]; one barrier
//   M6b one 16-lane DPP row per curve: summary_row_walk (summary_rows.h: curve_summary_kernel's walk and combine order, restated).  Lane j < 8
//       of the row owns functional j.  Factual arm: the value into ff[Q*C][8] and into the factual triple.  Arm v: the value into the cf
//       triple of v; e = fl(f_v - f_f) into the effect triple of v.  Slot 6 (t_hit): cf over the arm's crossing draws, effect over the draws
//       that cross in BOTH arms (its owner keeps the two counts per arm in the LDS); slot 7's effect is the difference of the indicators.
//   M7  once per trajectory: the owners store f [Q, B, C, 8], cf and eff [V, Q, B, C, 8] (the pinned order of fwd_moment_store_pinned)
// With f_* and eff_* all NULL the factual arm is skipped (workgroup-uniform).  Every output has ONE owner thread, which takes the draws in
// the fixed order; arm v touches nothing of another arm: column v is bitwise independent of V and of the other hypothesis rows, and the
// result is a function of (parameters, inputs, labels, hypotheses, noise, threshold) alone -- independent of the grid, of where the noise
// comes from and of which optional outputs are asked for; no atomics.  With no group intervened every arm runs the same operations on z_f:
// cf == f bitwise and every effect is exactly 0.
#include "slode_forward.h"
#include "summary_rows.h"

namespace {

constexpr int IS_NT = FWD_NT;
constexpr int IS_ROWS = IS_NT / 16;   // DPP rows of a workgroup: one per curve
static_assert(SLODE_MAX_HEADS * SLODE_MAX_C <= IS_ROWS, "one DPP row per curve");

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, the posterior loc | scale, the V
// counterfactual loc | scale rows, then the summary's own
struct IsLds { FwdLds f; LocScLds post; int cf, t, w, val, ff, mom, cnt; int total; };

struct IsK {
  FwdK f;
  PriorK pr;
  int ns, mask, V, has_thr, sense;
  const float *loc, *scale, *eps;
  float *f_mean, *f_sd, *cf_mean, *cf_sd, *eff_mean, *eff_sd;
  float thr[SLODE_MAX_C];
  IsLds o;
  RngK rng;
  LabelSrc lab;   // the batch's own label tensors
  LabelSrc hyp;   // hyp.p[i] == nullptr: label tensor i is not hypothesised (widths and offsets: lab's)
};

// column col of label row u'_{b,v}: row v of the hypothesis table of the tensor that holds the column, or the trajectory's own value
__device__ __forceinline__ float is_label_at(const LabelSrc& hyp, const LabelSrc& ls, long long b, int v, int col) {
  // (selects with compile-time indices: the kernel arguments are never indexed by a run-time value, which would copy them to scratch)
  const float *hp = hyp.p[0], *lp = ls.p[0];
  int lo = ls.off[0], hi = ls.off[1];
#pragma unroll
  for (int q = 1; q < SLODE_MAX_LABELS; ++q)
    if (q < ls.n && col >= ls.off[q]) { hp = hyp.p[q]; lp = ls.p[q]; lo = ls.off[q]; hi = ls.off[q + 1]; }
  const int w = hi - lo, c = col - lo;
  return hp ? hp[(long long)v * w + c] : lp[b * w + c];
}

// M7 of one triple in fwd_moment_store_pinned's operation order, each output only where it was asked for
__device__ __forceinline__ void is_store(const float* m, int P, float inv, float* mean, float* sd, long long o) {
#pragma clang fp contract(off)
  const float s1 = m[P], s2 = m[2 * P];
  if (mean) mean[o] = fmaf(s1, inv, m[0]);
  if (sd) {
    const float sq = s1 * s1, sub = sq * inv;
    sd[o] = sqrtf(fmaxf(s2 - sub, 0.f) * inv);
  }
}
__device__ __forceinline__ void is_store_nan(float* mean, float* sd, long long o) {
  const float nan = __builtin_nanf("");
  if (mean) mean[o] = nan;
  if (sd) sd[o] = nan;
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(IS_NT) intervene_summary_kernel(const IsK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_is[];
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.ns, V = k.V;
  const FwdSm sm = fwd_sm(s_is, k.o.f);   // (sm.u: u' of one arm at a time, only the columns of intervened groups are filled and read)
  float* s_loc = s_is + k.o.post.loc;    // posterior loc / scale
  float* s_sc = s_is + k.o.post.sc;
  float* s_cf = s_is + k.o.cf;           // [V][loc[L] | scale[L]] of the arms
  float* s_t = s_is + k.o.t;             // [T] the grid
  float* s_w = s_is + k.o.w;             // [T] trapezoid node weights
  float* s_val = s_is + k.o.val;         // [Q*C][T] the current arm's curves
  float* s_ff = s_is + k.o.ff;           // [Q*C][8] the current draw's factual functionals
  float* s_mom = s_is + k.o.mom;         // [1 + 2 V: factual | cf_0 | eff_0 | cf_1 | ...][3: v0, s1, s2][Q*C][8]
  int* s_cnt = reinterpret_cast<int*>(s_is + k.o.cnt);   // [Q*C][2 V: cf_v, eff_v] slot 6's draws so far (its owner's alone)
  const bool has_thr = k.has_thr != 0, above = k.sense > 0;
  const bool need_f = k.f_mean || k.f_sd || k.eff_mean || k.eff_sd;   // (workgroup-uniform)
  const bool need_e = k.eff_mean || k.eff_sd;
  const int P = QC * SLODE_SUMMARY_SLOTS;
  // M6b's roles: row <-> curve, lane of the row <-> stride-16 walk, then lanes 0..7 <-> functional
  const int row = tid >> 4, l16 = tid & 15;
  const bool row_on = row < QC;
  const int rq = row_on ? row / C : 0, rc = row_on ? row - rq * C : 0;
  const float row_thr = summary_thr(k.thr[0], k.thr[1], k.thr[2], k.thr[3], rc);
  const bool owner = row_on && l16 < SLODE_SUMMARY_SLOTS;
  const int own = row * SLODE_SUMMARY_SLOTS + l16;   // the owner's slot of a [Q*C][8] table

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  for (int t = tid; t < T; t += IS_NT) {
    s_t[t] = f.times[t];
    s_w[t] = 0.5f * (f.times[min(t + 1, T - 1)] - f.times[max(t - 1, 0)]);
  }
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- M1 ----
    __syncthreads();   // (M0's writes; the previous trajectory's readers of s_u / s_loc / s_sc / s_cf and its M6b)
    float loc = 0.f, sc = 0.f;
    if (tid < L) {
      loc = k.loc[(long long)b * L + tid]; sc = k.scale[(long long)b * L + tid];
      s_loc[tid] = loc; s_sc[tid] = sc;   // (read back by this thread alone)
    }
    for (int v = 0; v < V; ++v) {
      if (v) __syncthreads();   // (the previous arm's readers of s_u)
      if (tid < k.pr.nu) {
        int hit = 0;
        for (int g = 0; g < k.pr.n_groups; ++g)
          if (((k.mask >> g) & 1) && tid >= k.pr.grp[g].u_off && tid < k.pr.grp[g].u_off + k.pr.grp[g].u_dim) hit = 1;
        if (hit) sm.u[tid] = is_label_at(k.hyp, k.lab, b, v, tid);
      }
      __syncthreads();
      if (tid < L) {
        float cloc = loc, csc = sc, pl, pls;
        if (fwd_prior_at(k.pr, par, sm.u, tid, pl, pls, k.mask)) { cloc = pl; csc = expf(pls); }
        s_cf[v * 2 * L + tid] = cloc; s_cf[v * 2 * L + L + tid] = csc;   // (read back by this thread alone)
      }
    }
    int n_hit_f = 0;   // owner of slot 6: the factual arm's crossing draws so far
    for (int kk = 0; kk < ns; ++kk) {
      // draw kk = row kk * B + b of the call's noise: ONE value per latent dim, shared by all arms
      const float e = tid < L ? slode_eps_at(k.rng, k.eps, (long long)kk * f.B + b, L, tid) : 0.f;
      for (int arm = need_f ? -1 : 0; arm < V; ++arm) {
        // ---- M2 ----
        if (tid < L) sm.z[tid] = arm < 0 ? fmaf(s_sc[tid], e, s_loc[tid]) : fmaf(s_cf[arm * 2 * L + L + tid], e, s_cf[arm * 2 * L + tid]);
        __syncthreads();   // (also: the previous solve's readers of s_A / s_x0 / s_row[.][1] / s_val are done)
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
        // ---- M6a: head values of the thread's time points into the table ----
        for (int t = tid; t < T; t += IS_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, t, x);
          for (int qc = 0; qc < QC; ++qc) s_val[qc * T + t] = fwd_head_value<SM>(sm, S, qc, x);
        }
        __syncthreads();
        // ---- M6b: one DPP row per curve ----
        if (row_on) {
          const SummaryRow r = summary_row_walk(s_val + row * T, s_w, T, l16, has_thr, above, row_thr);
          if (l16 < SLODE_SUMMARY_SLOTS) {
            const bool crossed = r.ihit < T;
            const float fv = summary_slot_value(r, s_t, T, l16);
            if (arm < 0) {
              s_ff[own] = fv;   // (read by this thread, and slot 7 by slot 6's owner: the arms' barriers lie between)
              float* m = s_mom + own;
              if (l16 != 6) fwd_moment_add(m, P, kk == 0, fv);
              else if (crossed) { fwd_moment_add(m, P, n_hit_f == 0, fv); ++n_hit_f; }
            } else {
              float* m = s_mom + (1 + 2 * arm) * 3 * P + own;
              int* n = s_cnt + (row * V + arm) * 2;
              if (l16 != 6) {
                fwd_moment_add(m, P, kk == 0, fv);
                if (need_e) fwd_moment_add(m + 3 * P, P, kk == 0, fv - s_ff[own]);
              } else {
                const int n_cf = kk == 0 ? 0 : n[0], n_both = kk == 0 ? 0 : n[1];
                const bool both = need_e && crossed && s_ff[own + 1] != 0.f;
                if (crossed) fwd_moment_add(m, P, n_cf == 0, fv);
                if (both) fwd_moment_add(m + 3 * P, P, n_both == 0, fv - s_ff[own]);
                n[0] = n_cf + (crossed ? 1 : 0); n[1] = n_both + (both ? 1 : 0);
              }
            }
          }
        }
      }
    }
    // ---- M7: the owners' own values: no barrier needed ----
    if (owner) {
      const float inv = 1.0f / (float)ns;
      const long long of = (((long long)rq * f.B + b) * C + rc) * SLODE_SUMMARY_SLOTS + l16;
      const bool dead = l16 >= 5 && !has_thr;
      if (need_f) {
        const float* m = s_mom + own;
        if (dead || (l16 == 6 && n_hit_f == 0)) is_store_nan(k.f_mean, k.f_sd, of);
        else is_store(m, P, l16 == 6 ? 1.0f / (float)n_hit_f : inv, k.f_mean, k.f_sd, of);
      }
      for (int v = 0; v < V; ++v) {
        const long long o = ((((long long)v * f.Q + rq) * f.B + b) * C + rc) * SLODE_SUMMARY_SLOTS + l16;
        const float* m = s_mom + (1 + 2 * v) * 3 * P + own;
        const int n_cf = l16 == 6 ? s_cnt[(row * V + v) * 2] : 1, n_both = (l16 == 6 && need_e) ? s_cnt[(row * V + v) * 2 + 1] : 1;
        if (dead || n_cf == 0) is_store_nan(k.cf_mean, k.cf_sd, o);
        else is_store(m, P, l16 == 6 ? 1.0f / (float)n_cf : inv, k.cf_mean, k.cf_sd, o);
        if (need_e) {
          if (dead || n_both == 0) is_store_nan(k.eff_mean, k.eff_sd, o);
          else is_store(m + 3 * P, P, l16 == 6 ? 1.0f / (float)n_both : inv, k.eff_mean, k.eff_sd, o);
        }
      }
    }
  }
}

IsLds is_lds(const slode_shape& s, int V, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3, QC = Q * s.C;
  LdsCarve cv;
  IsLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.post = fwd_lds_loc_sc(cv, s);
  o.cf = cv.take(2 * s.L * V);
  o.t = cv.take(s.T); o.w = cv.take(s.T); o.val = cv.take(QC * s.T);
  o.ff = cv.take(QC * SLODE_SUMMARY_SLOTS);
  o.mom = cv.take(3 * QC * SLODE_SUMMARY_SLOTS * (1 + 2 * V));
  o.cnt = cv.take(QC * 2 * V);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_intervene_summary_lds_bytes(const slode_shape& s, int V, int force_generic) {
  return (size_t)is_lds(s, V, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_intervene_summary(const InterveneSummaryLaunch& a, hipStream_t stream) {
  const DrawsLaunch& d = a.d;
  const slode_shape& s = d.s;
  if (a.V < 1 || a.V > SLODE_INTERVENE_SUMMARY_MAX_ARMS || d.num_samples < 1 || d.grid < 1 || !a.cf_mean || (a.group_mask != 0 && d.lab.n < 1))
    return hipErrorInvalidValue;
  const size_t lds = slode_intervene_summary_lds_bytes(s, a.V, d.force_generic);
  if (lds > SLODE_INTERVENE_SUMMARY_LDS_MAX) return hipErrorInvalidValue;
  IsK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay);
  k.ns = d.num_samples; k.mask = (int)a.group_mask; k.V = a.V; k.has_thr = a.has_thr; k.sense = a.sense;
  k.loc = d.loc; k.scale = d.scale; k.eps = d.eps;
  k.f_mean = a.f_mean; k.f_sd = a.f_sd; k.cf_mean = a.cf_mean; k.cf_sd = a.cf_sd; k.eff_mean = a.eff_mean; k.eff_sd = a.eff_sd;
  for (int c = 0; c < SLODE_MAX_C; ++c) k.thr[c] = a.thr[c];
  k.rng = d.rng; k.lab = d.lab;
  k.hyp = d.lab;   // widths and offsets as the batch's
  for (int i = 0; i < SLODE_MAX_LABELS; ++i) k.hyp.p[i] = i < d.lab.n ? a.hyp[i] : nullptr;
  k.o = is_lds(s, a.V, fwd_generic(s, d.force_generic));
  fwd_dispatch(s, d.force_generic, [&](auto sc) { fwd_launch("intervene_summary", intervene_summary_kernel<decltype(sc)::value>, d.grid, lds, stream, k); });
  return hipGetLastError();
}
