// Latent attribution (slode_latent_attribution): per trajectory, how much of the variance of every decoder head curve comes from which block
// of the latent vector -- a prior group, or the rest dims no group covers -- over num_samples PICK-FREEZE draws, without writing anything
// sized num_samples x B x C x T.  Every draw has TWO noise rows, e (base) and e' (fresh):
//   base    z   = loc + scale * e                                                (the draw of recon_moments_kernel on the same side)
//   arm a   z_a = loc + scale * (l in a block of arm_masks[a] ? e'[l] : e[l])    (the blocks of the mask redrawn, the others frozen)
// and per arm the Jansen estimator msd[a] = 1 / (2 ns) sum_k (v_a,k - v_k)^2 of every head value: a single block in the mask estimates that
// block's total-effect variance, every block but one in the mask gives the first-order variance of the one left out as sd^2 - msd.
// The frame is that of intervene_moments_kernel, with A arms instead of one and a second noise row instead of a second label
// set.  One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1:
//   M0  once per workgroup: fwd_stage_weights -- every solve of every arm of every draw reuses them; the thread's block index (thread <-> dim)
//   M1  once per trajectory: fwd_draw_source
//   per draw: the thread's two noise values (row k * B + b of drawing calls n and n + 1, or of the explicit [2, ns, B, L] tensor), kept in
//   registers across all arms
//   per arm (the base as the arm with an empty mask, then the A arms): M2 z from the arm's mask; M3-M5 fwd_solve over the whole grid;
//   M6  thread <-> time point: the Q * C head values v.  Base: kept in the LDS (vf[Q*C][T], the thread's own slots) and added to the base
//       moments (fwd_moment_add).  Arm a: d = v - vf, s[a][qc][t] = fma(d, d, s)
//   M7  once per trajectory: fwd_moment_store of the base; msd = 0.5 s / ns, written with T contiguous
// Every value (the base moments, the kept base values, the sums of squares) belongs to ONE thread for the whole trajectory, which takes the
// draws in the fixed order k = 0 .. ns - 1: no atomics, no merge; the result is a function of (parameters, inputs, labels, noise, the arm's
// own mask) alone -- independent of the grid, of where the noise comes from and of which other arms are in the call.  An arm with an empty
// mask runs the base's instructions on the base's z: exactly 0.
#include "slode_forward.h"

namespace {

constexpr int AT_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct AtLds { FwdLds f; int acc, vf, arms; LocScLds ls; int total; };

struct AtK {
  DrawsK d;
  int n_arms;
  unsigned int masks[SLODE_ATTRIBUTION_MAX_ARMS];
  float *mean, *sd, *msd;
  AtLds o;
};

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(AT_NT) attribution_kernel(const AtK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_at[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.d.ns, A = k.n_arms;
  const FwdSm sm = fwd_sm(s_at, k.o.f);
  float* s_acc = s_at + k.o.acc;     // [Q*C][3: v0, s1, s2][T]: the base moments
  float* s_vf = s_at + k.o.vf;       // [Q*C][T]: the base head values of the current draw
  float* s_arm = s_at + k.o.arms;    // [A][Q*C][T]: sum over the draws of (v_a - v)^2
  float* s_loc = s_at + k.o.ls.loc;
  float* s_sc = s_at + k.o.ls.sc;

  // ---- M0: the weights every solve reuses; the block of the thread's latent dim: its prior group, else the rest block (bit n_groups) ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  int blk = k.d.pr.n_groups;
  for (int g = 0; g < k.d.pr.n_groups; ++g)
    if (tid >= k.d.pr.grp[g].z_off && tid < k.d.pr.grp[g].z_off + k.d.pr.grp[g].z_dim) blk = g;

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1
    for (int kk = 0; kk < ns; ++kk) {
      // draw kk = row kk * B + b of both noise sources: base and fresh, ONE value each per latent dim, shared by all arms
      const long long row = (long long)kk * f.B + b;
      float e0 = 0.f, e1 = 0.f;
      if (tid < L) {
        e0 = slode_eps_at(k.d.rng, k.d.eps, row, L, tid);
        e1 = slode_eps_at(k.d.rng, k.d.eps, row, L, tid, 1, (long long)ns * f.B);
      }
      for (int arm = -1; arm < A; ++arm) {
        const unsigned int mask = arm < 0 ? 0u : k.masks[arm];
        // ---- M2 ----
        if (tid < L) sm.z[tid] = fmaf(s_sc[tid], ((mask >> blk) & 1u) ? e1 : e0, s_loc[tid]);
        __syncthreads();   // (also: the previous solve's readers of s_A / s_x0 / s_row[.][1] are done)
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
        // ---- M6: head values of the thread's time points; base: kept, running moments; arm: the squared paired difference ----
        for (int t = tid; t < T; t += AT_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, t, x);
          for (int qc = 0; qc < QC; ++qc) {
            const float v = fwd_head_value<SM>(sm, S, qc, x);
            if (arm < 0) {
              s_vf[qc * T + t] = v;
              fwd_moment_add(s_acc + (qc * 3) * T + t, T, kk == 0, v);
            } else {
              float* s = s_arm + ((long long)arm * QC + qc) * T + t;
              const float dv = v - s_vf[qc * T + t];
              *s = fmaf(dv, dv, kk == 0 ? 0.f : *s);
            }
          }
        }
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    const float inv = 1.0f / (float)ns;
    for (int t = tid; t < T; t += AT_NT)
      for (int qc = 0; qc < QC; ++qc) {
        const int q = qc / C, c = qc - q * C;
        const long long o = (((long long)q * f.B + b) * C + c) * T + t;
        fwd_moment_store(s_acc + (qc * 3) * T + t, T, inv, k.mean, k.sd, o);
        for (int a = 0; a < A; ++a)
          k.msd[(long long)a * f.Q * f.B * C * T + o] = 0.5f * s_arm[((long long)a * QC + qc) * T + t] * inv;
      }
  }
}

AtLds at_lds(const slode_shape& s, int n_arms, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  AtLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 3 * s.T); o.vf = cv.take(Q * s.C * s.T); o.arms = cv.take(n_arms * Q * s.C * s.T);
  o.ls = fwd_lds_loc_sc(cv, s);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_attribution_lds_bytes(const slode_shape& s, int n_arms, int force_generic) {
  return (size_t)at_lds(s, n_arms, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_attribution(const AttributionLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  if (a.n_arms < 1 || a.n_arms > SLODE_ATTRIBUTION_MAX_ARMS || !a.msd || a.d.num_samples < 1 || a.d.grid < 1) return hipErrorInvalidValue;
  AtK k{};
  fwd_fill(k.d, a.d);
  k.n_arms = a.n_arms;
  for (int i = 0; i < a.n_arms; ++i) k.masks[i] = a.masks[i];
  k.mean = a.mean; k.sd = a.sd; k.msd = a.msd; k.o = at_lds(s, a.n_arms, fwd_generic(s, a.d.force_generic));
  const size_t lds = slode_attribution_lds_bytes(s, a.n_arms, a.d.force_generic);
  if (lds > SLODE_ATTRIBUTION_LDS_MAX) return hipErrorInvalidValue;
  fwd_dispatch(s, a.d.force_generic, [&](auto sc) { fwd_launch("latent_attribution", attribution_kernel<decltype(sc)::value>, a.d.grid, lds, stream, k); });
  return hipGetLastError();
}
