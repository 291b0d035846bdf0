// Calibration pass (slode_calibration): per COHORT, how the three curves of every family lie against the observations -- for each curve
// v_j (ALD: the heads mu_50, mu_75, mu_25; Gauss: mean, mean + 2 s, mean - 2 s with s = softplus(constant_std)) the number of (member, draw)
// pairs with y < v_j, the pairs inside the band [v_2, v_1), the pairs whose curves cross, the mean pinball loss and the mean band width.
// The draws are those of slode_recon_moments / slode_cohort_moments.  Three launches:
//   cohort_plan        the plan kernel of cohort_moments_kernel.hip, as it stands: the chunk table and the per-cohort partial ranges
//   calibration        one workgroup of four waves walks one chunk -- R consecutive members of ONE cohort -- at a time (persistent loop over
//                      the chunk ids) and writes one partial:
//     M0-M5 are the draw loop of slode_forward.h, a member in the place of the trajectory; once per workgroup the scale
//     table s[c][t] from the parameters (Gauss); per member the observation row is staged into [C][T] in memory order
//     M6'' thread <-> time point: the state, the Q head values, the three curves; the five indicators into int32 slots [5][C][T] and
//          the four summands (pinball 0..2, width), formed in fp32, into fp64 slots [4][C][T] -- lanes <-> t at unit stride, ONE owner thread
//          per slot from zeroing to store
//     the partial: the fp64 sums and the counts, plain per-lane stores, t contiguous, by the owner threads
//   calibration_merge  one workgroup per (cohort, channel), thread <-> (slice, time point): the cohort's partials in four contiguous slices,
//                      each added in slot order and the slices in a fixed order, counts in integer arithmetic, sums in fp64; the sums
//                      over t by the fixed tree of cohort_merge
// No atomics.  The counts are integers: a function of (parameters, inputs, noise, members, offsets) alone, whatever the grid AND the chunk.
// The float outputs are a function of those and the chunk.  A member index outside [0, B) is never used as an address: it flags its chunk,
// and the merge gives its cohort the empty value (counts 0, floats NaN); a NaN curve value flags its chunk and turns the cohort's floats NaN.
#include "slode_forward.h"

namespace {

constexpr int CA_NT = FWD_NT;
constexpr int CA_NI = 5, CA_NF = 4;   // count slots: below 0..2, inside, cross; sum slots: pinball 0..2, width

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then the fp64 sums [4][C][T] (8-byte aligned),
// the counts [5][C][T], the observations [C][T], the scale table [C][T] (Gauss) and loc / scale
struct CaLds { FwdLds f; int acc, cnt, obs, sig; LocScLds ls; int total; };

struct CaK {
  DrawsK d;
  int M, G, t_major, gauss, cstd;
  long long sb, PS;   // floats between observation rows; bytes of one partial
  float tau[3];
  const float* obs;
  const int *members, *cs;
  const int4* tab;
  int* flags;
  char* part;
  CaLds o;
};

// (y - v)(tau - [y < v]) in fp32; below = [y < v]
__device__ __forceinline__ float ca_pinball(float y, float v, float tau, bool below) { return (y - v) * (below ? tau - 1.f : tau); }

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(CA_NT) calibration_kernel(const CaK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_ca[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, ns = k.d.ns, CT = C * T;
  const int NCH = k.cs[k.G];
  if ((int)blockIdx.x >= NCH) return;   // (the grid is sized by the bound ceil(M / R) + G)
  const FwdSm sm = fwd_sm(s_ca, k.o.f);
  double* s_acc = reinterpret_cast<double*>(s_ca + k.o.acc);   // [4][C][T]
  int* s_cnt = reinterpret_cast<int*>(s_ca + k.o.cnt);         // [5][C][T]
  float* s_obs = s_ca + k.o.obs;                               // [C][T]
  float* s_sig = s_ca + k.o.sig;                               // [C][T] (Gauss)
  float* s_loc = s_ca + k.o.ls.loc;
  float* s_sc = s_ca + k.o.ls.sc;

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  if (k.gauss)
    for (int e = tid; e < CT; e += CA_NT) s_sig[e] = softplusf(f.params[k.cstd + e]);

  for (int i = blockIdx.x; i < NCH; i += gridDim.x) {
    const int4 ch = k.tab[i];   // cohort, first position, length
    int bad = 0, nan = 0;
    for (int t = tid; t < T; t += CA_NT) {   // the thread's own slots
      for (int j = 0; j < CA_NI * C; ++j) s_cnt[j * T + t] = 0;
      for (int j = 0; j < CA_NF * C; ++j) s_acc[j * T + t] = 0.0;
    }
    for (int j = 0; j < ch.z; ++j) {
      const int pos = min(max(ch.y + j, 0), k.M - 1);
      const int b = k.members[pos];
      if (b < 0 || b >= f.B) { bad = 1; continue; }   // (workgroup-uniform: never an address)
      fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1 (its first barrier: the previous member's readers of s_obs are done)
      {
        const float* __restrict__ y = k.obs + (long long)b * k.sb;   // (dense row: consecutive lanes, consecutive addresses)
        for (int e = tid; e < CT; e += CA_NT) s_obs[k.t_major ? (e % C) * T + e / C : e] = y[e];
      }
      for (int kk = 0; kk < ns; ++kk) {
        fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
        __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done; s_obs / s_sig are visible)
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
        // ---- M6'': the curves of the thread's time points against the staged observations ----
        for (int t = tid; t < T; t += CA_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, t, x);
          for (int c = 0; c < C; ++c) {
            const float y = s_obs[c * T + t];
            const float v0 = fwd_head_value<SM>(sm, S, c, x);
            float v1, v2;
            if (k.gauss) {
              const float w = 2.f * s_sig[c * T + t];
              v1 = v0 + w; v2 = v0 - w;
            } else {
              v1 = fwd_head_value<SM>(sm, S, C + c, x); v2 = fwd_head_value<SM>(sm, S, 2 * C + c, x);
            }
            const bool b0 = y < v0, b1 = y < v1, b2 = y < v2;   // (comparisons: false on NaN)
            int* n = s_cnt + c * T + t;
            n[0] += b0; n[CT] += b1; n[2 * CT] += b2;
            n[3 * CT] += (v2 <= y) && b1;
            n[4 * CT] += (v2 > v0) || (v0 > v1);
            double* a = s_acc + c * T + t;
            a[0] += (double)ca_pinball(y, v0, k.tau[0], b0);
            a[CT] += (double)ca_pinball(y, v1, k.tau[1], b1);
            a[2 * CT] += (double)ca_pinball(y, v2, k.tau[2], b2);
            a[3 * CT] += (double)(v1 - v2);
            nan |= (v0 != v0) || (v1 != v1) || (v2 != v2);
          }
        }
      }
    }
    // ---- the partial: the thread's own slots, lanes <-> consecutive t ----
    double* pd = reinterpret_cast<double*>(k.part + (long long)i * k.PS);
    int* pi = reinterpret_cast<int*>(pd + CA_NF * CT);
    for (int t = tid; t < T; t += CA_NT) {
      for (int j = 0; j < CA_NF * C; ++j) pd[j * T + t] = s_acc[j * T + t];
      for (int j = 0; j < CA_NI * C; ++j) pi[j * T + t] = s_cnt[j * T + t];
    }
    const int any_nan = __syncthreads_or(nan);
    if (tid == 0) k.flags[i] = bad | (any_nan ? 2 : 0);
  }
}

// ---- calibration_merge ----------------------------------------------------------------------------------------------
struct CgK {
  int G, C, T, K;
  long long PS;
  const int* cs;
  const int4* tab;
  const int* flags;
  const char* part;
  int *below, *inside, *cross;
  float *pinball, *width;
};

// 1024 threads: thread <-> (slice, time point of a round of 256).  A cohort's partials [p0, p1) are cut into CG_SL contiguous slices of
// ceil(n / CG_SL); every slice is added in slot order, the slices as ((s0 + s1) + s2) + s3 by the threads of slice 0, which write the outputs
constexpr int CG_SL = 4, CG_NT = CA_NT * CG_SL;

__global__ void __launch_bounds__(CG_NT) calibration_merge_kernel(const CgK k) {
  __shared__ double s_f[CG_SL - 1][CA_NF][CA_NT];
  __shared__ int s_i[CG_SL - 1][CA_NI][CA_NT];
  __shared__ double s_w[CA_NF][CA_NT / 64];
  __shared__ int s_n[CG_NT / 64];
  const int tid = threadIdx.x, tl = tid & (CA_NT - 1), sl = tid / CA_NT, lane = tid & 63, wave = tl >> 6;
  const int g = blockIdx.x / k.C, c = blockIdx.x - g * k.C, T = k.T, C = k.C, CT = C * T;
  const int p0 = k.cs[g], p1 = k.cs[g + 1];
  // the member count and the flags of the cohort: thread <-> partial, then integer sums over the workgroup
  int nm = 0, fl = 0;
  for (int p = p0 + tid; p < p1; p += CG_NT) { nm += k.tab[p].z; fl |= k.flags[p]; }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) nm += __shfl_xor(nm, off, 64);
  if (lane == 0) s_n[tid >> 6] = nm;
  const int bad = __syncthreads_or(fl & 1), nan = __syncthreads_or(fl & 2);   // (barriers: s_n is visible)
  long long N = 0;
  for (int w = 0; w < CG_NT / 64; ++w) N += s_n[w];
  const bool none = N == 0 || bad;
  const int q = (p1 - p0 + CG_SL - 1) / CG_SL, pa = min(p0 + sl * q, p1), pb = min(pa + q, p1);
  double sum[CA_NF] = {0.0, 0.0, 0.0, 0.0};
  for (int t0 = 0; t0 < T; t0 += CA_NT) {   // (workgroup-uniform)
    const int t = t0 + tl;
    int n[CA_NI] = {0, 0, 0, 0, 0};
    double a[CA_NF] = {0.0, 0.0, 0.0, 0.0};
    if (t < T) {
#pragma unroll 4
      for (int p = pa; p < pb; ++p) {
        const double* pd = reinterpret_cast<const double*>(k.part + (long long)p * k.PS);
        const int* pi = reinterpret_cast<const int*>(pd + CA_NF * CT);
#pragma unroll
        for (int j = 0; j < CA_NI; ++j) n[j] += pi[(j * C + c) * T + t];
#pragma unroll
        for (int j = 0; j < CA_NF; ++j) a[j] += pd[(j * C + c) * T + t];
      }
    }
    if (sl > 0) {
#pragma unroll
      for (int j = 0; j < CA_NI; ++j) s_i[sl - 1][j][tl] = n[j];
#pragma unroll
      for (int j = 0; j < CA_NF; ++j) s_f[sl - 1][j][tl] = a[j];
    }
    __syncthreads();
    if (sl == 0 && t < T) {
#pragma unroll
      for (int s = 0; s < CG_SL - 1; ++s) {
#pragma unroll
        for (int j = 0; j < CA_NI; ++j) n[j] += s_i[s][j][tl];
#pragma unroll
        for (int j = 0; j < CA_NF; ++j) a[j] += s_f[s][j][tl];
      }
      const long long o = ((long long)g * C + c) * T + t;
#pragma unroll
      for (int j = 0; j < 3; ++j) k.below[(long long)j * k.G * CT + o] = none ? 0 : n[j];
      if (k.inside) k.inside[o] = none ? 0 : n[3];
      if (k.cross) k.cross[o] = none ? 0 : n[4];
#pragma unroll
      for (int j = 0; j < CA_NF; ++j) sum[j] += a[j];
    }
    __syncthreads();   // (the next round writes s_i / s_f again)
  }
  if (k.pinball || k.width) {   // (workgroup-uniform) the sums over t: per thread t = tl, tl + 256, ..; then a fixed tree over lanes and waves
    if (sl == 0) {   // (whole waves)
#pragma unroll
      for (int j = 0; j < CA_NF; ++j) {
        double v = sum[j];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_w[j][wave] = v;
      }
    }
    __syncthreads();
    if (tid == 0) {
      const float fnan = __builtin_nanf("");
      const bool off = none || nan;
      const double den = (double)N * (double)k.K * (double)T;
      for (int j = 0; j < CA_NF; ++j) {
        const double tot = ((s_w[j][0] + s_w[j][1]) + s_w[j][2]) + s_w[j][3];
        const float r = off ? fnan : (float)(tot / den);
        if (j < 3) { if (k.pinball) k.pinball[((long long)j * k.G + g) * C + c] = r; }
        else if (k.width) k.width[g * C + c] = r;
      }
    }
  }
}

CaLds ca_lds(const slode_shape& s, bool generic) {
  const int CT = s.C * s.T;
  LdsCarve cv;
  CaLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(2 * CA_NF * CT); o.cnt = cv.take(CA_NI * CT); o.obs = cv.take(CT);
  o.sig = cv.take(s.likelihood == SLODE_GAUSS ? CT : 0); o.ls = fwd_lds_loc_sc(cv, s);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_calibration_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)ca_lds(s, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_calibration(const CalibrationLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  const CohortPart& c = a.c;
  const CohortScratch sc = slode_cohort_scratch(c.M, c.G, c.chunk, slode_calibration_partial_bytes(s));
  const size_t lds = slode_calibration_lds_bytes(s, a.d.force_generic);
  if (lds > SLODE_CALIBRATION_LDS_MAX || a.d.num_samples < 1 || a.d.grid < 1 || c.chunk < 1 || c.chunk > SLODE_COHORT_MAX_CHUNK || c.G < 1 ||
      c.G > SLODE_COHORT_MAX_G || c.M < 0 || c.M > s.B || !a.below || !c.obs || !c.scratch || (c.M > 0 && (!c.members || !c.offsets)))
    return hipErrorInvalidValue;
  char* base = (char*)c.scratch;
  int* cs = (int*)(base + sc.cs);
  int4* tab = (int4*)(base + sc.tab);
  int* flags = (int*)(base + sc.flags);
  char* part = base + sc.part;
  (void)slode_launch_cohort_plan(c.offsets, c.M, c.G, c.chunk, sc.n_partials, cs, tab, stream);
  CaK k{};
  fwd_fill(k.d, a.d);
  k.M = c.M; k.G = c.G; k.t_major = c.t_major; k.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; k.cstd = a.d.lay.cstd;
  k.sb = c.sb; k.PS = (long long)sc.partial_bytes;
  if (k.gauss) { k.tau[0] = 0.5f; k.tau[1] = SLODE_CALIBRATION_PHI2; k.tau[2] = SLODE_CALIBRATION_PHIM2; }
  else { k.tau[0] = 0.5f; k.tau[1] = 0.5f + s.quantile_diff; k.tau[2] = 0.5f - s.quantile_diff; }
  k.obs = c.obs; k.members = c.members; k.cs = cs; k.tab = tab; k.flags = flags; k.part = part;
  k.o = ca_lds(s, fwd_generic(s, a.d.force_generic));
  fwd_dispatch(s, a.d.force_generic, [&](auto scv) { fwd_launch("calibration", calibration_kernel<decltype(scv)::value>, a.d.grid, lds, stream, k); });
  CgK m{};
  m.G = c.G; m.C = s.C; m.T = s.T; m.K = a.d.num_samples; m.PS = (long long)sc.partial_bytes;
  m.cs = cs; m.tab = tab; m.flags = flags; m.part = part;
  m.below = a.below; m.inside = a.inside; m.cross = a.cross; m.pinball = a.pinball; m.width = a.width;
  SLODE_LAUNCH("calibration_merge", calibration_merge_kernel, dim3(c.G * s.C), dim3(CG_NT), 0, stream, m);
  return hipGetLastError();
}
