// Simultaneous (sup-t) credible bands (slode_joint_band): per trajectory, head curve and channel, the level-quantiles over num_samples = K latent
// draws of the draw's largest standardised deviation  dev_k = max_t |v_k(t) - mean(t)| / sd(t)  -- the ONE number per curve that turns
// mean +- crit sd into a band which holds the whole curve with the stated probability -- plus the share of draws wholly inside the pointwise
// band mean +- z sd and the deviation of the observed curve.  A functional of every draw's whole curve that needs mean and sd first: two
// sweeps over the same noise, nothing sized K x B x C x T anywhere.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid).  The frame is recon_moments_kernel's, the
// draw loop of slode_forward.h:
//   M0  once per workgroup: fwd_stage_weights
//   M1  once per trajectory: fwd_draw_source
//   sweep 1, per draw k = 0 .. K - 1: M2 fwd_draw_z, M3-M5 fwd_solve, M6 thread <-> time point: fwd_moment_add into the table [Q*C][3][T] --
//       recon_moments_kernel's loop unchanged.  At its end the owner of (q, c, t) forms mean and sd with fwd_moment_store IN PLACE (slot 0: m,
//       slot 1: s; the bits slode_recon_moments returns), stores them, and writes the observation's deviation |y - m| / s into slot 2, from
//       now on the value table val[Q*C][T]; one barrier; one 16-lane DPP row per curve reduces it to obs_dev and counts the points with
//       s > sd_floor.
//   sweep 2, per draw k = 0 .. K - 1 on the SAME noise (fwd_draw_z with the same k: explicit eps or the counter-based generator), M3-M5 again:
//     M6a thread <-> time point: e = |v - m| / s into val, subtraction and division each rounded on its own; -1 where s <= sd_floor (no maximum
//         selects it); one barrier
//     M6b one DPP row per curve: lane l walks t = l, l + 16, ...; the row maximum in four DPP steps (xor 1, xor 2, half mirror, mirror); lane 0
//         writes dev[curve][k] (0 for a curve without a participating point) into the LDS table [Q*C][K]
//   M7  once per trajectory: thread <-> (curve, draw): the rank of dev_k among the curve's K deviations by counting (ties broken by the draw
//       index, so the ranks are a permutation); the draw whose rank is r_j - 1 stores crit[j]; thread <-> (curve, level): joint[j] = #{dev_k <=
//       z_j} / K.  dev_out, when asked for, is the table itself.
// A maximum and an order statistic are selections: their order changes no bit.  Every output has ONE owner thread and the draws are taken in
// the fixed order: the result is a function of (parameters, inputs, noise, levels, sd_floor) alone -- bitwise independent of the grid and of
// where the noise comes from, no atomics.  Non-finite curve values are not ordered: the outputs of such a curve are unspecified.
#include "slode_forward.h"

namespace {

constexpr int JB_NT = FWD_NT;
constexpr int JB_ROWS = JB_NT / 16;   // DPP rows of a workgroup: one per curve
constexpr int JB_LV = SLODE_JOINT_BAND_MAX_LEVELS;
static_assert(SLODE_MAX_HEADS * SLODE_MAX_C <= JB_ROWS, "one DPP row per curve");

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, the moment table (slot 2: the value table of
// sweep 2), the deviations, loc | scale
struct JbLds { FwdLds f; int acc, dev; LocScLds ls; int total; };

struct JbK {
  DrawsK d;
  float *mean, *sd, *crit, *joint, *obs_dev, *dev_out;
  const float* obs;   // dense rows of C * T floats, or NULL
  int t_major, n_levels;
  float sd_floor;
  int r[JB_LV];     // ranks, counted from 1
  float z[JB_LV];   // pointwise half-widths
  JbLds o;
};

// the standardised deviation of one value with its operation order pinned -- the difference and the quotient each rounded on their own,
// a true division -- so that the result is bitwise the numpy restatement (tests/band_util.py), whatever the compiler would fuse;
// -1: the point does not take part
__device__ __forceinline__ float jb_dev(float v, float m, float s, float sd_floor) {
#pragma clang fp contract(off)
  const float d = fabsf(v - m);
  return s > sd_floor ? d / s : -1.f;
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(JB_NT) joint_band_kernel(const JbK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_jb[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.d.ns, n_levels = k.n_levels;
  const FwdSm sm = fwd_sm(s_jb, k.o.f);
  float* s_acc = s_jb + k.o.acc;   // [Q*C][3][T]: sweep 1: v0, s1, s2; afterwards m, s, val
  float* s_dev = s_jb + k.o.dev;   // [Q*C][K]
  float* s_loc = s_jb + k.o.ls.loc;
  float* s_sc = s_jb + k.o.ls.sc;
  const float sd_floor = k.sd_floor;
  const bool has_obs = k.obs != nullptr;
  // the row roles: row <-> curve, lane of the row <-> stride-16 walk
  const int row = tid >> 4, l16 = tid & 15;
  const bool row_on = row < QC;
  const int rq = row_on ? row / C : 0, rc = row_on ? row - rq * C : 0;

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1 (its first barrier: the previous trajectory's readers of s_dev / s_acc are done)
    // ---- sweep 1: recon_moments_kernel's draw loop ----
    for (int kk = 0; kk < ns; ++kk) {
      fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
      __syncthreads();
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
      for (int t = tid; t < T; t += JB_NT) {
        float x[SM];
        fwd_state_at<SM>(sm, S, t, x);
        for (int qc = 0; qc < QC; ++qc) fwd_moment_add(s_acc + (qc * 3) * T + t, T, kk == 0, fwd_head_value<SM>(sm, S, qc, x));
      }
    }
    // ---- its end: the thread's own (q, c, t): mean, sd in place and stored; the observation's deviation into the value slot ----
    const float inv = 1.0f / (float)ns;
    const float* __restrict__ y_row = has_obs ? k.obs + (long long)b * C * T : nullptr;
    for (int t = tid; t < T; t += JB_NT)
      for (int qc = 0; qc < QC; ++qc) {
        const int q = qc / C, c = qc - q * C;
        float* mt = s_acc + (qc * 3) * T + t;
        fwd_moment_store(mt, T, inv, mt, mt + T, 0);   // slot 0 <- mean, slot 1 <- sd (it reads s1, s2, v0 before it writes)
        const float m = mt[0], s = mt[T];
        const long long o = (((long long)q * f.B + b) * C + c) * T + t;
        k.mean[o] = m; k.sd[o] = s;
        mt[2 * T] = has_obs ? jb_dev(y_row[k.t_major ? t * C + c : c * T + t], m, s, sd_floor) : -1.f;
      }
    __syncthreads();
    if (row_on && k.obs_dev) {
      const float* v_row = s_acc + (row * 3 + 2) * T;
      const float* s_row = s_acc + (row * 3 + 1) * T;
      float mx = -1.f;
      int np = 0;
      for (int t = l16; t < T; t += 16) {
        const float e = v_row[t];
        mx = e > mx ? e : mx;
        np += s_row[t] > sd_floor ? 1 : 0;
      }
      mx = row16_max(mx);
      np = row16_sum_i(np);
      if (l16 == 0) {
        const long long o = (((long long)rq * f.B + b) * C + rc) * 2;
        k.obs_dev[o] = has_obs ? (mx < 0.f ? 0.f : mx) : __builtin_nanf("");
        k.obs_dev[o + 1] = (float)np;
      }
    }
    // ---- sweep 2: the same noise, the same solves; the deviations of every draw ----
    for (int kk = 0; kk < ns; ++kk) {
      fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
      __syncthreads();   // (also: the readers of the value slot -- the observation's row, the previous draw's M6b -- are done)
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
      // ---- M6a: the thread's time points ----
      for (int t = tid; t < T; t += JB_NT) {
        float x[SM];
        fwd_state_at<SM>(sm, S, t, x);
        for (int qc = 0; qc < QC; ++qc) {
          float* mt = s_acc + (qc * 3) * T + t;
          mt[2 * T] = jb_dev(fwd_head_value<SM>(sm, S, qc, x), mt[0], mt[T], sd_floor);
        }
      }
      __syncthreads();
      // ---- M6b: one DPP row per curve ----
      if (row_on) {
        const float* v_row = s_acc + (row * 3 + 2) * T;
        float mx = -1.f;
        int t = l16;
        for (; t + 48 < T; t += 64) {   // four points per trip, their LDS reads issued together
          const float e0 = v_row[t], e1 = v_row[t + 16], e2 = v_row[t + 32], e3 = v_row[t + 48];
          mx = e0 > mx ? e0 : mx; mx = e1 > mx ? e1 : mx; mx = e2 > mx ? e2 : mx; mx = e3 > mx ? e3 : mx;
        }
        for (; t < T; t += 16) { const float e = v_row[t]; mx = e > mx ? e : mx; }
        mx = row16_max(mx);
        if (l16 == 0) s_dev[row * ns + kk] = mx < 0.f ? 0.f : mx;
      }
    }
    __syncthreads();
    // ---- M7: thread <-> (curve, draw): its rank by counting; the deviations are >= +0, so their bit patterns order as they do ----
    for (int item = tid; item < QC * ns; item += JB_NT) {
      const int qc = item / ns, kk = item - qc * ns;
      const int q = qc / C, c = qc - q * C;
      const float* dv = s_dev + qc * ns;
      const float mine_f = dv[kk];
      const int mine = __float_as_int(mine_f);
      int rank = 0;
      for (int i = 0; i < ns; ++i) {
        const int o = __float_as_int(dv[i]);
        rank += (o < mine || (o == mine && i < kk)) ? 1 : 0;
      }
      const long long base = ((long long)q * f.B + b) * C + c;
#pragma unroll
      for (int j = 0; j < JB_LV; ++j)   // (a compile-time index: the kernel arguments are never indexed by a run-time value)
        if (j < n_levels && k.r[j] - 1 == rank) k.crit[base * n_levels + j] = mine_f;
      if (k.dev_out) k.dev_out[base * ns + kk] = mine_f;
    }
    if (k.joint)
      for (int item = tid; item < QC * n_levels; item += JB_NT) {
        const int qc = item / n_levels, j = item - qc * n_levels;
        const int q = qc / C, c = qc - q * C;
        const float* dv = s_dev + qc * ns;
        float zj = 0.f;
#pragma unroll
        for (int jj = 0; jj < JB_LV; ++jj) zj = jj == j ? k.z[jj] : zj;
        int cnt = 0;
        for (int i = 0; i < ns; ++i) cnt += dv[i] <= zj ? 1 : 0;
        k.joint[(((long long)q * f.B + b) * C + c) * n_levels + j] = (float)cnt / (float)ns;
      }
  }
}

JbLds jb_lds(const slode_shape& s, int ns, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  JbLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 3 * s.T);
  o.dev = cv.take(Q * s.C * ns);
  o.ls = fwd_lds_loc_sc(cv, s);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_joint_band_lds_bytes(const slode_shape& s, int num_samples, int force_generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  if (num_samples < 1 || (long long)Q * s.C * num_samples > (1 << 26)) return (size_t)1 << 30;   // (far beyond any budget; keeps the carve's int arithmetic in range)
  return (size_t)jb_lds(s, num_samples, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_joint_band(const JointBandLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  const int K = a.d.num_samples;
  if (K < 2 || a.d.grid < 1 || !a.mean || !a.sd || !a.crit || a.n_levels < 1 || a.n_levels > JB_LV || !(a.sd_floor >= 0.f)) return hipErrorInvalidValue;
  const size_t lds = slode_joint_band_lds_bytes(s, K, a.d.force_generic);
  if (lds > SLODE_JOINT_BAND_LDS_MAX) return hipErrorInvalidValue;
  JbK k{};
  fwd_fill(k.d, a.d);
  k.mean = a.mean; k.sd = a.sd; k.crit = a.crit; k.joint = a.joint; k.obs_dev = a.obs_dev; k.dev_out = a.dev_out;
  k.obs = a.obs; k.t_major = a.t_major; k.n_levels = a.n_levels; k.sd_floor = a.sd_floor;
  for (int j = 0; j < JB_LV; ++j) {
    const bool on = j < a.n_levels;
    k.r[j] = on ? a.rank[j] : 0; k.z[j] = on ? a.z[j] : 0.f;
    if (on && (k.r[j] < 1 || k.r[j] > K)) return hipErrorInvalidValue;
  }
  k.o = jb_lds(s, K, fwd_generic(s, a.d.force_generic));
  fwd_dispatch(s, a.d.force_generic, [&](auto sc) { fwd_launch("joint_band", joint_band_kernel<decltype(sc)::value>, a.d.grid, lds, stream, k); });
  return hipGetLastError();
}
