// The row walk of the curve summaries (M6b of DESIGN 3.20) as an inline routine: one 16-lane DPP row per curve.  Lane l walks the points
// t = l, l + 16, ... in increasing order and keeps (max, first index), (min, first index), the fma sum of w v, the sum of w [beyond] and the
// first index beyond; the row combines in four DPP steps (xor 1, xor 2, half mirror, mirror: row16_sum's order; an extreme prefers the
// smaller index on a tie), after which every lane of the row holds the same seven values.
// This is curve_summary_kernel.hip's M6b restated operation for operation -- the same trapezoid weights, the same four-point trips, the same
// combine order, the same tie rule -- so that a kernel which calls it writes that kernel's bits (tests/test_gpu_intervene_summary.py holds the
// two against each other with torch.equal).  curve_summary_kernel.hip keeps its own copy: its code object is left as it is.
// Included by intervene_summary_kernel.hip and forecast_summary_kernel.hip; the latter walks a curve window by window and merges the windows'
// rows with the routines at the end of this file.
#pragma once
#include "slode_common.h"

namespace {

// thr[c] by selects among four values read once: the kernel arguments are never indexed by a run-time value
__device__ __forceinline__ float summary_thr(float t0, float t1, float t2, float t3, int c) { return c == 0 ? t0 : (c == 1 ? t1 : (c == 2 ? t2 : t3)); }

// the extreme of a row with the smallest index attaining it: GT: the maximum, else the minimum.  Both partners of a step see the same pair of
// (value, index) and pick the same one, so after the four steps every lane of the row holds the row's.
template <bool GT, int CTRL>
__device__ __forceinline__ void summary_ext_step(float& v, int& i) {
  const float ov = dpp_f<CTRL>(v);
  const int oi = dpp_i<CTRL>(i);
  const bool take = (GT ? ov > v : ov < v) || (ov == v && oi < i);
  v = take ? ov : v; i = take ? oi : i;
}
template <bool GT>
__device__ __forceinline__ void summary_row_ext(float& v, int& i) {
  summary_ext_step<GT, 0xB1>(v, i); summary_ext_step<GT, 0x4E>(v, i); summary_ext_step<GT, 0x141>(v, i); summary_ext_step<GT, 0x140>(v, i);
}

// what every lane of a row holds after the walk: an index equal to T: no point (ihit: the curve does not cross)
struct SummaryRow { float vmax, vmin, auc, tb; int imax, imin, ihit; };

// v_row: the curve's T values; s_w: the node weights; l16: the lane of the row.  Call with all 16 lanes of the row active.
__device__ __forceinline__ SummaryRow summary_row_walk(const float* v_row, const float* s_w, int T, int l16, bool has_thr, bool above, float row_thr) {
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
  summary_row_ext<true>(vmax, imax);
  summary_row_ext<false>(vmin, imin);
  auc = row16_sum(auc);
  tb = row16_sum(tb);
  ihit = row16_min_i(ihit);
  return SummaryRow{vmax, vmin, auc, tb, imax, imin, ihit};
}

// functional `slot` (0 .. 7) of the row; slot 6 of a curve that does not cross is t[T - 1] and must not be used
__device__ __forceinline__ float summary_slot_value(const SummaryRow& r, const float* s_t, int T, int slot) {
  switch (slot) {
    case 0: return r.vmax;
    case 1: return s_t[min(r.imax, T - 1)];
    case 2: return r.vmin;
    case 3: return s_t[min(r.imin, T - 1)];
    case 4: return r.auc;
    case 5: return r.tb;
    case 6: return s_t[min(r.ihit, T - 1)];
    default: return r.ihit < T ? 1.f : 0.f;
  }
}

// ---- a curve walked in several windows (forecast_summary_kernel.hip) ----
// What a row carries across the windows of one curve: the extremes so far with the TIME of the first point that attained them, the running
// trapezoid sums, the time of the first point beyond the threshold.  Every lane of the row holds the same values.
struct SummaryCarry { float vmax, tmax, vmin, tmin, auc, tb, thit; bool hit; };

__device__ __forceinline__ SummaryCarry summary_carry_init() {
  return SummaryCarry{-INFINITY, 0.f, INFINITY, 0.f, 0.f, 0.f, 0.f, false};
}

// The SummaryRow r of a window's n >= 1 walked points into the carry; t_w: the times of those points (r's indices count from its first one).
// Windows arrive in increasing time order: an extreme moves on STRICT improvement only, so the earliest point wins a tie across windows as
// it does inside one; auc and time_beyond add in window order; the first hit stays once it is set.  A lane of a window shorter than the row
// holds the sentinels (-inf / +inf, n) before the combine and loses every step to a lane with a point, so r's indices are < n here.
__device__ __forceinline__ void summary_merge(SummaryCarry& c, const SummaryRow& r, const float* t_w, int n) {
  if (r.vmax > c.vmax) { c.vmax = r.vmax; c.tmax = t_w[min(r.imax, n - 1)]; }
  if (r.vmin < c.vmin) { c.vmin = r.vmin; c.tmin = t_w[min(r.imin, n - 1)]; }
  c.auc += r.auc;
  c.tb += r.tb;
  if (!c.hit && r.ihit < n) { c.hit = true; c.thit = t_w[r.ihit]; }
}

// functional `slot` (0 .. 7) of the carry after the last window; slot 6 of a curve that does not cross must not be used
__device__ __forceinline__ float summary_carry_value(const SummaryCarry& c, int slot) {
  switch (slot) {
    case 0: return c.vmax;
    case 1: return c.tmax;
    case 2: return c.vmin;
    case 3: return c.tmin;
    case 4: return c.auc;
    case 5: return c.tb;
    case 6: return c.thit;
    default: return c.hit ? 1.f : 0.f;
  }
}

}  // namespace
