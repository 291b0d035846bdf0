// Sample moments of the reconstruction (slode_recon_moments): per trajectory, the mean and the population standard deviation over
// num_samples latent draws of every decoder head curve -- what the reference's evaluation takes from `multiple_samples` (np.mean / np.std
// over the sample axis) -- without writing anything sized num_samples x B x C x T.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in
// that order.  This kernel is the draw loop of slode_forward.h and nothing else:
//   M0  once per workgroup: fwd_stage_weights -- every draw of every trajectory reuses them
//   M1  once per trajectory: fwd_draw_source
//   per draw: M2 fwd_draw_z, M3-M5 fwd_solve over the whole grid
//   M6  thread <-> time point: the Q * C head values and their running moments (fwd_moment_add), table [Q*C][3][T]
//   M7  once per trajectory: fwd_moment_store, written with T contiguous
// The moments of (q, c, t) belong to ONE thread for the whole trajectory and take the draws in the fixed order k = 0 .. ns - 1: the
// result is a function of (parameters, inputs, noise) alone -- independent of the grid, bitwise reproducible, no atomics.
#include "slode_forward.h"

namespace {

constexpr int RM_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then the moments and loc | scale
struct RmLds { FwdLds f; int acc; LocScLds ls; int total; };

struct RmK {
  DrawsK d;
  float *mean, *sd;
  RmLds o;
};

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(RM_NT) recon_moments_kernel(const RmK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_rm[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.d.ns;
  const FwdSm sm = fwd_sm(s_rm, k.o.f);
  float* s_acc = s_rm + k.o.acc;   // [Q*C][3: v0, s1, s2][T]
  float* s_loc = s_rm + k.o.ls.loc;
  float* s_sc = s_rm + k.o.ls.sc;

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1
    for (int kk = 0; kk < ns; ++kk) {
      fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
      // ---- M6: head values of the thread's time points, running moments ----
      for (int t = tid; t < T; t += RM_NT) {
        float x[SM];
        fwd_state_at<SM>(sm, S, t, x);
        for (int qc = 0; qc < QC; ++qc) fwd_moment_add(s_acc + (qc * 3) * T + t, T, kk == 0, fwd_head_value<SM>(sm, S, qc, x));
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    const float inv = 1.0f / (float)ns;
    for (int t = tid; t < T; t += RM_NT)
      for (int qc = 0; qc < QC; ++qc) {
        const int q = qc / C, c = qc - q * C;
        fwd_moment_store(s_acc + (qc * 3) * T + t, T, inv, k.mean, k.sd, (((long long)q * f.B + b) * C + c) * T + t);
      }
  }
}

RmLds rm_lds(const slode_shape& s, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  RmLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 3 * s.T); o.ls = fwd_lds_loc_sc(cv, s);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_recon_moments_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)rm_lds(s, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_recon_moments(const ReconMomentsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  RmK k{};
  fwd_fill(k.d, a.d);
  k.mean = a.mean; k.sd = a.sd; k.o = rm_lds(s, fwd_generic(s, a.d.force_generic));
  const size_t lds = slode_recon_moments_lds_bytes(s, a.d.force_generic);
  if (lds > SLODE_RECON_MOMENTS_LDS_MAX || a.d.num_samples < 1 || a.d.grid < 1) return hipErrorInvalidValue;
  fwd_dispatch(s, a.d.force_generic, [&](auto sc) { fwd_launch("recon_moments", recon_moments_kernel<decltype(sc)::value>, a.d.grid, lds, stream, k); });
  return hipGetLastError();
}
