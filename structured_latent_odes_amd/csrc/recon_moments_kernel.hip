// Sample moments of the reconstruction (slode_recon_moments): per trajectory, the mean and the population standard deviation over
// num_samples latent draws of every decoder head curve -- what the reference's evaluation takes from `multiple_samples` (np.mean / np.std
// over the sample axis) -- without writing anything sized num_samples x B x C x T.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in
// that order:
// The forward phases M0, M3-M5 and the prior nets of M1 are the shared ones of slode_forward.h.
//   M0  once per workgroup: [w_t | u_j | W_g | W_d] per hidden unit, the z-columns of the hidden layer and the init net (transposed), the
//       init net's output layer, the head weights and the biases into the LDS -- every draw of every trajectory reuses them
//   M1  once per trajectory: labels; loc / scale of the posterior (from the encoder launch) or of the conditional prior nets, N(0, 1) on
//       the dims outside every prior group (as phase E0 of eval_stats_kernel forms z3)
//   per draw:
//   M2  z = loc + scale * eps_k (row k * B + b of ONE drawing call, or of the explicit [ns, B, L] tensor)
//   M3  time-invariant part of the hidden layer (into the unit's weight row) and the init net; x0
//   M4  step coefficients x' = A x + b of every grid step (tests/kernel_math.py step_coeffs), thread <-> step, weights from the LDS
//   M5  forward affine scan (one solve on all four waves): one state component per wave pass
//   M6  thread <-> time point: the Q * C head values v and the running moments of (q, c, t), shifted by the first draw's value v0:
//       s1 += v - v0, s2 += (v - v0)^2 -- no sum of v^2, whose fp32 rounding would exceed the variance of a prior-pass curve
//   M7  once per trajectory: mean = v0 + s1 / ns, sd = sqrt(max(0, s2 - s1^2 / ns) / ns), written with T contiguous
// The moments of (q, c, t) belong to ONE thread for the whole trajectory and take the draws in the fixed order k = 0 .. ns - 1: the
// result is a function of (parameters, inputs, noise) alone -- independent of the grid, bitwise reproducible, no atomics.
#include "slode_forward.h"

namespace {

constexpr int RM_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then the moments and loc / scale
struct RmLds { FwdLds f; int acc, loc, sc, total; };

struct RmK {
  FwdK f;
  PriorK pr;
  int is_post, ns;
  const float *loc, *scale, *eps, *u;
  float *mean, *sd;
  RmLds o;
  RngK rng;
  LabelSrc lab;
};

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(RM_NT) recon_moments_kernel(const RmK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_rm[];
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, H = f.H, C = f.C, NS = T - 1, QC = f.Q * C, ns = k.ns;
  const FwdSm sm = fwd_sm(s_rm, k.o.f);
  float* s_acc = s_rm + k.o.acc;   // [Q*C][3: v0, s1, s2][T]
  float* s_loc = s_rm + k.o.loc;
  float* s_sc = s_rm + k.o.sc;

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
    for (int kk = 0; kk < ns; ++kk) {
      // ---- M2: draw kk = row kk * B + b of the call's noise ----
      if (tid < L) sm.z[tid] = fmaf(s_sc[tid], slode_eps_at(k.rng, k.eps, (long long)kk * f.B + b, L, tid), s_loc[tid]);
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
      // ---- M3: u = W_z z + b_h into the units' rows; the init net's hidden layer ----
      fwd_init_state<SM>(sm, H, L, S, tid);
      // ---- M4: step coefficients ----
      fwd_step_table_staged<SM>(f, sm, S, tid);
      __syncthreads();
      // ---- M5: forward affine scan, in place: x[n + 1][s] takes the slot of A[n][s] ----
      fwd_scan(sm.A, sm.B, sm.x0, S, NS, lane, wave, RM_NT / 64);
      __syncthreads();
      // ---- M6: head values of the thread's time points, running moments ----
      for (int t = tid; t < T; t += RM_NT) {
        float x[SM];
#pragma unroll
        for (int s = 0; s < SM; ++s) x[s] = s < S ? (t == 0 ? sm.x0[s] : sm.A[(t - 1) * S + s]) : 0.f;
        for (int qc = 0; qc < QC; ++qc) {
          float v = 0.f;
#pragma unroll
          for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(sm.hw[qc * S + s], x[s], v);
          float* m = s_acc + (qc * 3) * T + t;
          if (kk == 0) { m[0] = v; m[T] = 0.f; m[2 * T] = 0.f; }
          else { const float dv = v - m[0]; m[T] += dv; m[2 * T] = fmaf(dv, dv, m[2 * T]); }
        }
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    {
      const float inv = 1.0f / (float)ns;
      for (int t = tid; t < T; t += RM_NT)
        for (int qc = 0; qc < QC; ++qc) {
          const int q = qc / C, c = qc - q * C;
          const float* m = s_acc + (qc * 3) * T + t;
          const float s1 = m[T], s2 = m[2 * T];
          const long long o = (((long long)q * f.B + b) * C + c) * T + t;
          k.mean[o] = fmaf(s1, inv, m[0]);
          if (k.sd) k.sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
        }
    }
  }
}

RmLds rm_lds(const slode_shape& s, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  RmLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 3 * s.T); o.loc = cv.take(s.L); o.sc = cv.take(s.L);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_recon_moments_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)rm_lds(s, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_recon_moments(const ReconMomentsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  RmK k{};
  fwd_fill(k.f, s, lay, a.params, a.times, a.stage_t); fwd_fill(k.pr, s, lay);
  k.is_post = a.is_post; k.ns = a.num_samples;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u;
  k.mean = a.mean; k.sd = a.sd; k.rng = a.rng; k.lab = a.lab; k.o = rm_lds(s, fwd_generic(s, a.force_generic));
  const size_t lds = slode_recon_moments_lds_bytes(s, a.force_generic);
  if (lds > SLODE_RECON_MOMENTS_LDS_MAX || a.num_samples < 1 || a.grid < 1) return hipErrorInvalidValue;
  fwd_dispatch(s, a.force_generic, [&](auto sc) { fwd_launch("recon_moments", recon_moments_kernel<decltype(sc)::value>, a.grid, lds, stream, k); });
  return hipGetLastError();
}
