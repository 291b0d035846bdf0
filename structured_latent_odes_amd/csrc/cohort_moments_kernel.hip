// Cohort moments (slode_cohort_moments): per COHORT -- a set of trajectories of the batch, e.g. the subjects of one condition -- the mean, the
// population sd over members x draws, the population sd over the members of the per-member draw mean, the mean observation and the
// reference notebooks' L1 error of every decoder head curve, without writing anything per trajectory.  The draws are those of
// slode_recon_moments (row k * B + b of one drawing call, b the member's index in the batch).  Three launches:
//   cohort_plan     one workgroup: offsets[G + 1] -> the chunk table {cohort, first position, length} and the per-cohort partial ranges
//                   [cs[g], cs[g + 1]) by a block scan over ceil(n_g / R); offsets are clamped to [0, M], a decreasing pair is an empty cohort
//   cohort_moments  one workgroup of four waves folds one chunk -- R consecutive members of ONE cohort -- at a time (persistent loop over
//                   the chunk ids) and writes one partial:
//     M0-M5 are the draw loop of slode_forward.h, a member in the place of recon_moments_kernel's trajectory; per member its
//     observations are also added into [C][T]
//     M6' thread <-> time point: per (q, c) the value v (clipped) updates six floats in the LDS, shifted by v00, the chunk's first
//         member's first draw: t1 += dv, t2 += dv^2 (all values: fwd_moment_add), m1 += dv (this member); after the member's last draw mb = m1 / K,
//         b1 += mb, b2 += mb^2, m1 = 0 -- never a sum of v^2
//     the partial: v00, t1, t2, b1, b2 per value and the observation sum, plain per-lane stores, t contiguous, by the values' owner threads
//   cohort_merge    one workgroup per (cohort, channel), thread <-> time point: walks the cohort's partials in slot order, each as (count,
//                   mean, M2) of the values and of the member means in fp64, merged by Chan's pairwise update; the L1 sum over t in fp64 by
//                   a fixed-shape tree
// Every value has ONE owner thread which sees members and draws in list order; no atomics: the result is a function of (parameters,
// inputs, noise, members, offsets, chunk) alone, independent of the launch grid.  A member index outside [0, B) is never used as an
// address: it flags its chunk, and the merge turns every output of that cohort into NaN; positions are clamped to [0, M).
#include "slode_forward.h"

namespace {

constexpr int CM_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then the six-float table [Q*C][6][T], the
// observation sum [C][T] and loc / scale
struct CmLds { FwdLds f; int acc, obs; LocScLds ls; int total; };

struct CmK {
  DrawsK d;
  int M, G, t_major;
  long long sb, PS;   // floats between observation rows; floats of one partial
  float clip;
  const float* obs;
  const int *members, *cs;
  const int4* tab;
  int* flags;
  float* part;
  CmLds o;
};

// ---- cohort_plan ----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(CM_NT) cohort_plan_kernel(const int* __restrict__ offsets, int M, int G, int R, int NP, int* __restrict__ cs,
                                                           int4* __restrict__ tab) {
  __shared__ int s_o[SLODE_COHORT_MAX_G + 1];
  __shared__ int s_cs[SLODE_COHORT_MAX_G + 1];
  __shared__ long long s_sum[CM_NT];
  const int tid = threadIdx.x;
  for (int g = tid; g <= G; g += CM_NT) s_o[g] = M > 0 ? min(max(offsets[g], 0), M) : 0;
  __syncthreads();
  constexpr int PER = SLODE_COHORT_MAX_G / CM_NT;   // consecutive cohorts per thread
  long long own = 0;
  for (int j = 0; j < PER; ++j) {
    const int g = tid * PER + j;
    if (g < G) own += (max(s_o[g + 1] - s_o[g], 0) + R - 1) / R;
  }
  s_sum[tid] = own;
  __syncthreads();
  for (int off = 1; off < CM_NT; off <<= 1) {   // inclusive scan of the threads' sums
    const long long add = tid >= off ? s_sum[tid - off] : 0;
    __syncthreads();
    s_sum[tid] += add;
    __syncthreads();
  }
  long long run = s_sum[tid] - own;
  for (int j = 0; j < PER; ++j) {
    const int g = tid * PER + j;
    if (g <= G) s_cs[g] = (int)(run < NP ? run : NP);   // (never beyond the scratch, whatever offsets hold)
    if (g < G) run += (max(s_o[g + 1] - s_o[g], 0) + R - 1) / R;
  }
  if (tid == CM_NT - 1 && G == SLODE_COHORT_MAX_G) s_cs[G] = (int)(run < NP ? run : NP);
  __syncthreads();
  for (int g = tid; g <= G; g += CM_NT) cs[g] = s_cs[g];
  const int NCH = s_cs[G];
  for (int i = tid; i < NCH; i += CM_NT) {
    int lo = 0, hi = G - 1;   // the cohort whose range holds i: the largest g with cs[g] <= i
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_cs[mid] <= i) lo = mid; else hi = mid - 1;
    }
    const int j = i - s_cs[lo], n = max(s_o[lo + 1] - s_o[lo], 0);
    tab[i] = make_int4(lo, s_o[lo] + j * R, min(R, n - j * R), 0);
  }
}

// ---- cohort_moments -------------------------------------------------------------------------------------------------
// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(CM_NT) cohort_moments_kernel(const CmK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_cm[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.d.ns, CT = C * T;
  const int NCH = k.cs[k.G];
  if ((int)blockIdx.x >= NCH) return;   // (the grid is sized by the bound ceil(M / R) + G)
  const FwdSm sm = fwd_sm(s_cm, k.o.f);
  float* s_acc = s_cm + k.o.acc;   // [Q*C][6: v00, t1, t2, m1, b1, b2][T]
  float* s_obs = s_cm + k.o.obs;   // [C][T]
  float* s_loc = s_cm + k.o.ls.loc;
  float* s_sc = s_cm + k.o.ls.sc;

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0

  for (int i = blockIdx.x; i < NCH; i += gridDim.x) {
    const int4 ch = k.tab[i];   // cohort, first position, length
    float* part = k.part + (long long)i * k.PS;
    int bad = 0;
    bool first = true;
    // the observation sum: memory index e of a row <-> slot c * T + t, one owner thread per slot from here to the partial's store
    if (k.obs)
      for (int e = tid; e < CT; e += CM_NT) s_obs[k.t_major ? (e % C) * T + e / C : e] = 0.f;
    for (int j = 0; j < ch.z; ++j) {
      const int pos = min(max(ch.y + j, 0), k.M - 1);
      const int b = k.members[pos];
      if (b < 0 || b >= f.B) { bad = 1; continue; }   // (workgroup-uniform: never an address)
      fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1
      if (k.obs) {
        const float* __restrict__ y = k.obs + (long long)b * k.sb;   // (dense row: consecutive lanes, consecutive addresses)
        for (int e = tid; e < CT; e += CM_NT) s_obs[k.t_major ? (e % C) * T + e / C : e] += y[e];
      }
      for (int kk = 0; kk < ns; ++kk) {
        fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
        __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
        // ---- M6': head values of the thread's time points into the six-float table ----
        const bool init = first && kk == 0, last = kk == ns - 1;
        for (int t = tid; t < T; t += CM_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, t, x);
          for (int qc = 0; qc < QC; ++qc) {
            float v = fwd_head_value<SM>(sm, S, qc, x);
            if (v < k.clip) v = k.clip;   // (a comparison: NaN stays NaN)
            float* m = s_acc + (qc * 6) * T + t;
            const float dv = fwd_moment_add(m, T, init, v);   // slots 0 - 2: v00, t1, t2
            float m1 = 0.f;
            if (init) { m[4 * T] = 0.f; m[5 * T] = 0.f; }
            else m1 = m[3 * T] + dv;
            if (last) {
              const float mb = m1 / (float)ns;
              m[4 * T] += mb; m[5 * T] = fmaf(mb, mb, m[5 * T]); m1 = 0.f;
            }
            m[3 * T] = m1;
          }
        }
      }
      first = false;
    }
    // ---- the partial: the thread's own values, lanes <-> consecutive t ----
    for (int t = tid; t < T; t += CM_NT)
      for (int qc = 0; qc < QC; ++qc) {
        const float* m = s_acc + (qc * 6) * T + t;
        float* p = part + (long long)(qc * 5) * T + t;
        p[0] = m[0]; p[T] = m[T]; p[2 * T] = m[2 * T]; p[3 * T] = m[4 * T]; p[4 * T] = m[5 * T];
      }
    if (k.obs)
      for (int e = tid; e < CT; e += CM_NT) {
        const int slot = k.t_major ? (e % C) * T + e / C : e;
        part[(long long)5 * QC * T + slot] = s_obs[slot];
      }
    if (tid == 0) k.flags[i] = bad;
  }
}

// ---- cohort_merge ---------------------------------------------------------------------------------------------------
struct CgK {
  int G, C, T, Q, K, has_obs;
  long long PS;
  const int* cs;
  const int4* tab;
  const int* flags;
  const float* part;
  float *mean, *sd, *sdb, *obs_mean, *l1;
};

__global__ void __launch_bounds__(CM_NT) cohort_merge_kernel(const CgK k) {
  __shared__ double s_w[CM_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = blockIdx.x / k.C, c = blockIdx.x - g * k.C, T = k.T, C = k.C, QC = k.Q * k.C;
  const int p0 = k.cs[g], p1 = k.cs[g + 1];
  long long N = 0;
  int bad = 0;
  for (int p = p0; p < p1; ++p) { N += k.tab[p].z; bad |= k.flags[p]; }
  const bool none = N == 0 || bad;
  const float fnan = __builtin_nanf("");
  double l1 = 0.0;
  for (int t = tid; t < T; t += CM_NT) {
    float om = fnan;
    if (k.has_obs) {
      double so = 0.0;
      for (int p = p0; p < p1; ++p) so += (double)k.part[(long long)p * k.PS + (long long)5 * QC * T + c * T + t];
      if (!none) om = (float)(so / (double)N);
      if (k.obs_mean) k.obs_mean[((long long)g * C + c) * T + t] = om;
    }
    float m0 = fnan;
    for (int q = 0; q < k.Q; ++q) {
      const int qc = q * C + c;
      double nA = 0.0, meanA = 0.0, M2A = 0.0, mA = 0.0, meanbA = 0.0, M2bA = 0.0;   // values: (count, mean, M2); member means: the same
      for (int p = p0; p < p1; ++p) {
        const float* v = k.part + (long long)p * k.PS + (long long)(qc * 5) * T + t;
        const double n = (double)k.tab[p].z, nk = n * (double)k.K;
        const double v00 = v[0], t1 = v[T], t2 = v[2 * T], b1 = v[3 * T], b2 = v[4 * T];
        const double meanB = v00 + t1 / nk, M2B = nk > 1.0 ? fmax(t2 - t1 * t1 / nk, 0.0) : 0.0;
        const double meanbB = v00 + b1 / n, M2bB = n > 1.0 ? fmax(b2 - b1 * b1 / n, 0.0) : 0.0;
        {
          const double nn = nA + nk, d = meanB - meanA;
          meanA += d * (nk / nn); M2A += M2B + d * d * (nA * nk / nn); nA = nn;
        }
        {
          const double nn = mA + n, d = meanbB - meanbA;
          meanbA += d * (n / nn); M2bA += M2bB + d * d * (mA * n / nn); mA = nn;
        }
      }
      const long long o = (((long long)q * k.G + g) * C + c) * T + t;
      const float mean = none ? fnan : (float)meanA;
      k.mean[o] = mean;
      if (k.sd) k.sd[o] = none ? fnan : (float)sqrt(M2A / nA);
      if (k.sdb) k.sdb[o] = none ? fnan : (float)sqrt(M2bA / mA);
      if (q == 0) m0 = mean;
    }
    l1 += fabs((double)om - (double)m0);
  }
  if (k.l1) {   // (workgroup-uniform) the sum over t: per thread t = tid, tid + 256, ..; then a fixed tree over lanes and waves
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) l1 += __shfl_down(l1, off, 64);
    if (lane == 0) s_w[wave] = l1;
    __syncthreads();
    if (tid == 0) k.l1[g * C + c] = none ? fnan : (float)(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]);
  }
}

CmLds cm_lds(const slode_shape& s, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  CmLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(Q * s.C * 6 * s.T); o.obs = cv.take(s.C * s.T); o.ls = fwd_lds_loc_sc(cv, s);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_cohort_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)cm_lds(s, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_cohort_plan(const int32_t* offsets, int M, int G, int R, int NP, int* cs, void* tab, hipStream_t stream) {
  SLODE_LAUNCH("cohort_plan", cohort_plan_kernel, dim3(1), dim3(CM_NT), 0, stream, offsets, M, G, R, NP, cs, (int4*)tab);
  return hipGetLastError();
}

hipError_t slode_launch_cohort_moments(const CohortMomentsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  const CohortPart& c = a.c;
  const CohortScratch sc = slode_cohort_scratch(c.M, c.G, c.chunk, slode_cohort_partial_bytes(s));
  const size_t lds = slode_cohort_lds_bytes(s, a.d.force_generic);
  if (lds > SLODE_COHORT_LDS_MAX || a.d.num_samples < 1 || a.d.grid < 1 || c.chunk < 1 || c.chunk > SLODE_COHORT_MAX_CHUNK || c.G < 1 ||
      c.G > SLODE_COHORT_MAX_G || c.M < 0 || c.M > s.B || !a.mean || !c.scratch || (c.M > 0 && (!c.members || !c.offsets)))
    return hipErrorInvalidValue;
  char* base = (char*)c.scratch;
  int* cs = (int*)(base + sc.cs);
  int4* tab = (int4*)(base + sc.tab);
  int* flags = (int*)(base + sc.flags);
  float* part = (float*)(base + sc.part);
  (void)slode_launch_cohort_plan(c.offsets, c.M, c.G, c.chunk, sc.n_partials, cs, tab, stream);
  CmK k{};
  fwd_fill(k.d, a.d);
  k.M = c.M; k.G = c.G; k.t_major = c.t_major; k.sb = c.sb; k.PS = (long long)(sc.partial_bytes / sizeof(float)); k.clip = a.clip_min;
  k.obs = c.obs; k.members = c.members; k.cs = cs; k.tab = tab; k.flags = flags; k.part = part;
  k.o = cm_lds(s, fwd_generic(s, a.d.force_generic));
  fwd_dispatch(s, a.d.force_generic, [&](auto scv) { fwd_launch("cohort_moments", cohort_moments_kernel<decltype(scv)::value>, a.d.grid, lds, stream, k); });
  CgK m{};
  m.G = c.G; m.C = s.C; m.T = s.T; m.Q = k.d.f.Q; m.K = a.d.num_samples; m.has_obs = c.obs ? 1 : 0; m.PS = k.PS;
  m.cs = cs; m.tab = tab; m.flags = flags; m.part = part;
  m.mean = a.mean; m.sd = a.sd; m.sdb = a.sd_subjects; m.obs_mean = a.obs_mean; m.l1 = a.l1;
  SLODE_LAUNCH("cohort_merge", cohort_merge_kernel, dim3(c.G * s.C), dim3(CM_NT), 0, stream, m);
  return hipGetLastError();
}
