// Curve summaries (slode_curve_summary): per trajectory, head curve and channel, the mean and the population standard deviation over
// num_samples latent draws of eight functionals of the draw's WHOLE curve -- peak, time of peak, trough, time of trough, trapezoid area,
// time beyond a threshold, first time beyond it, whether it is crossed at all -- and, optionally, the share of draws beyond the threshold at
// every time point.  These are non-linear in the curve: none follows from the moments slode_recon_moments returns, and nothing sized
// num_samples x B x C x T is written to get them.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in that
// order.  The frame is recon_moments_kernel's, the draw loop of slode_forward.h:
//   M0  once per workgroup: fwd_stage_weights; the grid t[T] and the trapezoid node weights w[T] in fp32
//   M1  once per trajectory: fwd_draw_source
//   per draw: M2 fwd_draw_z, M3-M5 fwd_solve over the whole grid
//   M6a thread <-> time point: the Q * C head values into the table val[Q*C][T] -- the bits slode_recon_moments accumulates -- and the
//       thread's own int32 counters cnt[Q*C][T] of the points beyond the threshold; one barrier
//   M6b one 16-lane DPP row per curve: lane l walks t = l, l + 16, ... in increasing order and keeps (max, first index), (min, first index),
//       the fma sums of w v and of w [beyond] and the first index beyond; the row combines in four DPP steps (xor 1, xor 2, half mirror,
//       mirror: row16_sum's order; an extreme prefers the smaller index on a tie), after which every lane holds all eight functionals.
//       Lane j < 8 of the row owns the shifted moment triple of functional j (fwd_moment_add); slot 6 (t_hit) takes the crossing draws only.
//   M7  once per trajectory: the owners store mean / sd [Q, B, C, 8] (fwd_moment_store_pinned); the threads of M6a store p_beyond = cnt / ns with T contiguous
// The summation tree of auc and time_beyond is therefore fixed: per lane a left-to-right fma chain over its points, then
// ((l ^ 1) pair) -> ((l ^ 2) pair) -> half mirror -> mirror, each step adding two values that both partners hold, so every lane of the row ends
// with the same bits.  Every output has ONE owner thread, which takes the draws in the fixed order: the result is a function of (parameters,
// inputs, noise, threshold) alone -- independent of the grid and of where the noise comes from, bitwise reproducible, no atomics.
#include "slode_forward.h"

namespace {

constexpr int CS_NT = FWD_NT;
constexpr int CS_ROWS = CS_NT / 16;   // DPP rows of a workgroup: one per curve, Q * C <= SLODE_MAX_HEADS * SLODE_MAX_C = 12 of them busy
static_assert(SLODE_MAX_HEADS * SLODE_MAX_C <= CS_ROWS, "one DPP row per curve");

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, loc | scale, then the kernel's own
struct CsLds { FwdLds f; LocScLds ls; int t, w, val, cnt, mom; int total; };

struct CsK {
  DrawsK d;
  float *mean, *sd, *p_beyond;
  float thr[SLODE_MAX_C];
  int has_thr, sense;
  CsLds o;
};

// thr[c] by selects among four values read once: the kernel arguments are never indexed by a run-time value
__device__ __forceinline__ float cs_thr(float t0, float t1, float t2, float t3, int c) { return c == 0 ? t0 : (c == 1 ? t1 : (c == 2 ? t2 : t3)); }

// the extreme of a row with the smallest index attaining it: GT: the maximum, else the minimum.  Both partners of a step see the same pair of
// (value, index) and pick the same one, so after the four steps every lane of the row holds the row's.
template <bool GT, int CTRL>
__device__ __forceinline__ void cs_ext_step(float& v, int& i) {
  const float ov = dpp_f<CTRL>(v);
  const int oi = dpp_i<CTRL>(i);
  const bool take = (GT ? ov > v : ov < v) || (ov == v && oi < i);
  v = take ? ov : v; i = take ? oi : i;
}
template <bool GT>
__device__ __forceinline__ void cs_row_ext(float& v, int& i) {
  cs_ext_step<GT, 0xB1>(v, i); cs_ext_step<GT, 0x4E>(v, i); cs_ext_step<GT, 0x141>(v, i); cs_ext_step<GT, 0x140>(v, i);
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(CS_NT) curve_summary_kernel(const CsK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_cs[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.d.ns;
  const FwdSm sm = fwd_sm(s_cs, k.o.f);
  float* s_loc = s_cs + k.o.ls.loc;
  float* s_sc = s_cs + k.o.ls.sc;
  float* s_t = s_cs + k.o.t;                                  // [T] the grid: t_peak / t_trough / t_hit are read once per draw
  float* s_w = s_cs + k.o.w;                                  // [T] trapezoid node weights
  float* s_val = s_cs + k.o.val;                              // [Q*C][T] the current draw's curves
  int* s_cnt = reinterpret_cast<int*>(s_cs + k.o.cnt);        // [Q*C][T] draws beyond the threshold (only with p_beyond)
  float* s_mom = s_cs + k.o.mom;                              // [3: v0, s1, s2][Q*C][8]
  const bool has_thr = k.has_thr != 0, above = k.sense > 0, counts = k.p_beyond != nullptr;
  const int P = QC * SLODE_SUMMARY_SLOTS;
  // M6b's roles: row <-> curve, lane of the row <-> stride-16 walk, then lanes 0..7 <-> functional
  const int row = tid >> 4, l16 = tid & 15;
  const bool row_on = row < QC;
  const int rq = row_on ? row / C : 0, rc = row_on ? row - rq * C : 0;
  const float th0 = k.thr[0], th1 = k.thr[1], th2 = k.thr[2], th3 = k.thr[3];
  const float row_thr = cs_thr(th0, th1, th2, th3, rc);

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  for (int t = tid; t < T; t += CS_NT) {
    s_t[t] = f.times[t];
    s_w[t] = 0.5f * (f.times[min(t + 1, T - 1)] - f.times[max(t - 1, 0)]);
  }
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1 (its first barrier: s_t / s_w are visible; the previous trajectory's M6b is done)
    int n_hit = 0;                                   // owner of slot 6: the crossing draws so far
    for (int kk = 0; kk < ns; ++kk) {
      fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] / s_val are done)
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
      // ---- M6a: head values of the thread's time points into the table; the thread's own counters ----
      for (int t = tid; t < T; t += CS_NT) {
        float x[SM];
        fwd_state_at<SM>(sm, S, t, x);
        for (int qc = 0; qc < QC; ++qc) {
          const float v = fwd_head_value<SM>(sm, S, qc, x);
          s_val[qc * T + t] = v;
          if (counts) {
            const float th = cs_thr(th0, th1, th2, th3, qc - (qc / C) * C);
            const int hit = (above ? v > th : v < th) ? 1 : 0;
            s_cnt[qc * T + t] = kk == 0 ? hit : s_cnt[qc * T + t] + hit;
          }
        }
      }
      __syncthreads();
      // ---- M6b: one DPP row per curve ----
      if (row_on) {
        const float* v_row = s_val + row * T;
        float vmax = -INFINITY, vmin = INFINITY, auc = 0.f, tb = 0.f;
        int imax = T, imin = T, ihit = T;
        auto point = [&](float v, float w, int t) {
          if (v > vmax) { vmax = v; imax = t; }
          if (v < vmin) { vmin = v; imin = t; }
          auc = fmaf(w, v, auc);
          const bool hit = has_thr && (above ? v > row_thr : v < row_thr);
          tb += hit ? w : 0.f;
          ihit = (hit && ihit == T) ? t : ihit;
        };
        int t = l16;
        for (; t + 48 < T; t += 64) {   // four points per trip, their LDS reads issued together; the points still in increasing order
          const float v0 = v_row[t], v1 = v_row[t + 16], v2 = v_row[t + 32], v3 = v_row[t + 48];
          const float w0 = s_w[t], w1 = s_w[t + 16], w2 = s_w[t + 32], w3 = s_w[t + 48];
          point(v0, w0, t); point(v1, w1, t + 16); point(v2, w2, t + 32); point(v3, w3, t + 48);
        }
        for (; t < T; t += 16) point(v_row[t], s_w[t], t);
        cs_row_ext<true>(vmax, imax);
        cs_row_ext<false>(vmin, imin);
        auc = row16_sum(auc);
        tb = row16_sum(tb);
        ihit = row16_min_i(ihit);
        if (l16 < SLODE_SUMMARY_SLOTS) {
          const bool crossed = ihit < T;
          float fv;
          switch (l16) {
            case 0: fv = vmax; break;
            case 1: fv = s_t[min(imax, T - 1)]; break;
            case 2: fv = vmin; break;
            case 3: fv = s_t[min(imin, T - 1)]; break;
            case 4: fv = auc; break;
            case 5: fv = tb; break;
            case 6: fv = s_t[min(ihit, T - 1)]; break;
            default: fv = crossed ? 1.f : 0.f; break;
          }
          float* m = s_mom + row * SLODE_SUMMARY_SLOTS + l16;
          if (l16 != 6) fwd_moment_add(m, P, kk == 0, fv);
          else if (crossed) { fwd_moment_add(m, P, n_hit == 0, fv); ++n_hit; }
        }
      }
    }
    // ---- M7: the owners' own values: no barrier needed ----
    const float inv = 1.0f / (float)ns;
    if (row_on && l16 < SLODE_SUMMARY_SLOTS) {
      const long long o = (((long long)rq * f.B + b) * C + rc) * SLODE_SUMMARY_SLOTS + l16;
      const float* m = s_mom + row * SLODE_SUMMARY_SLOTS + l16;
      const float nan = __builtin_nanf("");
      if (l16 >= 5 && !has_thr) { k.mean[o] = nan; if (k.sd) k.sd[o] = nan; }
      else if (l16 != 6) fwd_moment_store_pinned(m, P, inv, k.mean, k.sd, o);
      else if (n_hit == 0) { k.mean[o] = nan; if (k.sd) k.sd[o] = nan; }
      else fwd_moment_store_pinned(m, P, 1.0f / (float)n_hit, k.mean, k.sd, o);
    }
    if (counts)
      for (int t = tid; t < T; t += CS_NT)
        for (int qc = 0; qc < QC; ++qc) {
          const int q = qc / C, c = qc - q * C;
          k.p_beyond[(((long long)q * f.B + b) * C + c) * T + t] = (float)s_cnt[qc * T + t] / (float)ns;
        }
  }
}

CsLds cs_lds(const slode_shape& s, bool want_p, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  CsLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.ls = fwd_lds_loc_sc(cv, s);
  o.t = cv.take(s.T); o.w = cv.take(s.T); o.val = cv.take(Q * s.C * s.T);
  o.cnt = want_p ? cv.take(Q * s.C * s.T) : o.val;
  o.mom = cv.take(3 * Q * s.C * SLODE_SUMMARY_SLOTS);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_curve_summary_lds_bytes(const slode_shape& s, int want_p_beyond, int force_generic) {
  return (size_t)cs_lds(s, want_p_beyond != 0, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_curve_summary(const CurveSummaryLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  CsK k{};
  fwd_fill(k.d, a.d);
  k.mean = a.mean; k.sd = a.sd; k.p_beyond = a.p_beyond; k.has_thr = a.has_thr; k.sense = a.sense;
  for (int c = 0; c < SLODE_MAX_C; ++c) k.thr[c] = a.thr[c];
  k.o = cs_lds(s, a.p_beyond != nullptr, fwd_generic(s, a.d.force_generic));
  const size_t lds = slode_curve_summary_lds_bytes(s, a.p_beyond != nullptr, a.d.force_generic);
  if (lds > SLODE_CURVE_SUMMARY_LDS_MAX || a.d.num_samples < 1 || a.d.grid < 1 || !a.mean || (a.p_beyond && !a.has_thr)) return hipErrorInvalidValue;
  fwd_dispatch(s, a.d.force_generic, [&](auto sc) { fwd_launch("curve_summary", curve_summary_kernel<decltype(sc)::value>, a.d.grid, lds, stream, k); });
  return hipGetLastError();
}
