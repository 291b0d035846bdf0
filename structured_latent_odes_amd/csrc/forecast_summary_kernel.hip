// Forecast summaries (slode_forecast_summary): per trajectory, head curve and channel, the mean and the population standard deviation over
// num_samples latent draws of the eight curve functionals of slode_curve_summary -- peak, time of peak, trough, time of trough, trapezoid
// area, time beyond a threshold, first time beyond it, whether it is crossed at all -- of the draw's curve on the output grid
// times_out[i0 .. T_out), i0 = first_point: "from here on".  The draws are those of slode_recon_moments, the solve is
// slode_forecast_moments' (the grid walked in windows of W steps, a carried state between them), the functionals are summary_rows.h's.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid).  DRAWS OUTER, WINDOWS INNER -- the
// reverse of forecast_moments_kernel, whose outputs are per time point and which therefore keeps a [ns][S] carry table: these outputs are
// per curve, so a draw is walked to the end of the grid before the next one starts and ONE [S] carry serves.  Nothing in the LDS is sized by
// num_samples or by T_out.
//   M0  once per workgroup: fwd_stage_weights (one window: also the grid t and the node weights w, which then never change)
//   M1  once per trajectory: fwd_draw_source
//   per draw: M2 fwd_draw_z, M3 fwd_init_state -- once, every window of the draw reads the same units' rows and x0
//   per window w -- steps [n_lo, n_hi), slots j = 0 .. nw with slot j = time point n_lo + j; slot 0 (x0) belongs to window 0 alone:
//   M4  fwd_step_table_staged on the window's steps
//   M5  fwd_scan from x0 (window 0) or from the carry; the state at the window's last point -> carry (forecast_moments_kernel's M3-M5
//       sequence for the same W: the states are that kernel's bits)
//   M6a thread <-> slot at or beyond i0: the Q * C head values into val[Q*C][W + 1]; with several windows also t and w of the slot,
//       w[g] = 0.5 (t[min(g + 1, T_out - 1)] - t[max(g - 1, i0)]): the trapezoid rule on the sub-grid; one barrier
//   M6b one 16-lane DPP row per curve: summary_row_walk on the window's slots at or beyond i0 (a window with none skips it: uniform in the
//       workgroup), then the window's SummaryRow merged into the draw's carry in the row's registers (summary_merge; every lane holds the
//       same values): an extreme moves on strict improvement only and takes its TIME along, auc and time_beyond add in window order, the
//       first hit stays once set
//   after the last window: lane j < 8 of the row adds functional j into its shifted moment triple (slot 6: the crossing draws only)
//   M7  once per trajectory: the owners store mean / sd [Q, B, C, 8] (fwd_moment_store_pinned)
// With one window, i0 = 0 and times_out = times every operation is curve_summary_kernel's: the result is bit for bit that call's.  The result
// is a function of (parameters, inputs, noise, output grid, i0, threshold, W) alone -- independent of the launch grid and of where the noise
// comes from, bitwise reproducible, no atomics; two windows agree to fp32 rounding (the scan's association; the fma chain's lanes).
#include "slode_forward.h"
#include "summary_rows.h"

namespace {

constexpr int FS_NT = FWD_NT;
constexpr int FS_ROWS = FS_NT / 16;   // DPP rows of a workgroup: one per curve
static_assert(SLODE_MAX_HEADS * SLODE_MAX_C <= FS_ROWS, "one DPP row per curve");

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones (A | b sized for W steps), loc | scale, the
// carry, then one window's grid, node weights and values, and the moment triples
struct FsLds { FwdLds f; LocScLds ls; int carry, t, w, val, mom; int total; };

struct FsK {
  DrawsK d;   // (d.f.T, times, stage_t: the OUTPUT grid)
  float *mean, *sd;
  float thr[SLODE_MAX_C];
  int has_thr, sense, W, i0;
  FsLds o;
};

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(FS_NT) forecast_summary_kernel(const FsK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_fs[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, NS = T - 1, ns = k.d.ns, W = k.W, PW = W + 1, i0 = k.i0;
  const FwdSm sm = fwd_sm(s_fs, k.o.f);
  float* s_loc = s_fs + k.o.ls.loc;
  float* s_sc = s_fs + k.o.ls.sc;
  float* s_carry = s_fs + k.o.carry;   // [S] the draw's state at the last point of the previous window
  float* s_t = s_fs + k.o.t;           // [W + 1] the window's grid times
  float* s_w = s_fs + k.o.w;           // [W + 1] the window's trapezoid node weights
  float* s_val = s_fs + k.o.val;       // [Q*C][W + 1] the current draw's curves on the window
  float* s_mom = s_fs + k.o.mom;       // [3: v0, s1, s2][Q*C][8]
  const bool has_thr = k.has_thr != 0, above = k.sense > 0;
  const bool one_w = W >= NS;          // (workgroup-uniform) the whole grid in one window: t and w are staged once
  const int P = QC * SLODE_SUMMARY_SLOTS;
  // M6b's roles: row <-> curve, lane of the row <-> stride-16 walk, then lanes 0..7 <-> functional
  const int row = tid >> 4, l16 = tid & 15;
  const bool row_on = row < QC;
  const int rq = row_on ? row / C : 0, rc = row_on ? row - rq * C : 0;
  const float row_thr = summary_thr(k.thr[0], k.thr[1], k.thr[2], k.thr[3], rc);
  auto node_w = [&](int g) { return 0.5f * (f.times[min(g + 1, T - 1)] - f.times[max(g - 1, i0)]); };

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  if (one_w)
    for (int t = tid; t < T; t += FS_NT) { s_t[t] = f.times[t]; s_w[t] = node_w(t); }
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1 (its first barrier: s_t / s_w are visible; the previous trajectory's M6b is done)
    int n_hit = 0;                                   // owner of slot 6: the crossing draws so far
    for (int kk = 0; kk < ns; ++kk) {
      fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] / s_val / s_t / s_w are done)
      fwd_init_state<SM>(sm, f.H, f.L, S, tid);   // M3, once per draw (x0 and the rows are visible after the first window's barrier)
      SummaryCarry cy = summary_carry_init();
      for (int n_lo = 0; n_lo < NS; n_lo += W) {
        const int n_hi = min(n_lo + W, NS), nw = n_hi - n_lo;
        const int j_lo = n_lo == 0 ? 0 : 1;   // the window's points: slots j_lo .. nw (slot 0: x0, window 0 alone)
        fwd_step_table_staged<SM>(f, sm, S, n_lo, n_hi, tid);   // M4
        __syncthreads();   // (also: the previous window's walk is done with s_val / s_t / s_w)
        fwd_scan(sm.A, sm.B, n_lo == 0 ? sm.x0 : s_carry, S, nw, lane, wave, FS_NT / 64);   // M5
        __syncthreads();
        if (tid < S) s_carry[tid] = sm.A[(nw - 1) * S + tid];   // (its next reader: the scan of the next window, two barriers on)
        // ---- M6a: head values of the thread's slots at or beyond i0 into the table; the slots' times and node weights ----
        const int off = max(j_lo, i0 - n_lo), cnt = nw + 1 - off;   // (workgroup-uniform; a window before i0: cnt <= 0, no slot)
        for (int j = off + tid; j <= nw; j += FS_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, j, x);
          for (int qc = 0; qc < QC; ++qc) s_val[qc * PW + j] = fwd_head_value<SM>(sm, S, qc, x);
          if (!one_w) { const int g = n_lo + j; s_t[j] = f.times[g]; s_w[j] = node_w(g); }
        }
        __syncthreads();
        // ---- M6b: one DPP row per curve, the same slots ----
        if (cnt > 0 && row_on) {
          const SummaryRow r = summary_row_walk(s_val + row * PW + off, s_w + off, cnt, l16, has_thr, above, row_thr);
          summary_merge(cy, r, s_t + off, cnt);
        }
      }
      if (row_on && l16 < SLODE_SUMMARY_SLOTS) {
        float* m = s_mom + row * SLODE_SUMMARY_SLOTS + l16;
        const float fv = summary_carry_value(cy, l16);
        if (l16 != 6) fwd_moment_add(m, P, kk == 0, fv);
        else if (cy.hit) { fwd_moment_add(m, P, n_hit == 0, fv); ++n_hit; }
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
  }
}

// the pieces for a window of W steps: fwd_lds on a shape whose T is the window's point count gives A | b of W S floats each
FsLds fs_lds(const slode_shape& s, int W, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3, QC = Q * s.C;
  slode_shape sw = s;
  sw.T = W + 1;
  LdsCarve cv;
  FsLds o{};
  o.f = fwd_lds(cv, sw, generic);
  o.ls = fwd_lds_loc_sc(cv, s);
  o.carry = cv.take(s.S);
  o.t = cv.take(W + 1); o.w = cv.take(W + 1); o.val = cv.take(QC * (W + 1));
  o.mom = cv.take(3 * QC * SLODE_SUMMARY_SLOTS);
  o.total = cv.n;
  return o;
}

}  // namespace

// W <= SLODE_FORECAST_MAX_T keeps every piece inside an int (the callers' range; the result is compared with the budget)
size_t slode_forecast_summary_lds_bytes(const slode_shape& s, int window, int force_generic) {
  return (size_t)fs_lds(s, window, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_forecast_summary(const ForecastSummaryLaunch& a, hipStream_t stream) {
  const DrawsLaunch& d = a.d;
  const slode_shape& s = d.s;
  if (d.num_samples < 1 || d.grid < 1 || a.T_out < 2 || a.window < 1 || a.window > a.T_out - 1 || a.first_point < 0 || a.first_point > a.T_out - 1 ||
      !a.mean)
    return hipErrorInvalidValue;
  const size_t lds = slode_forecast_summary_lds_bytes(s, a.window, d.force_generic);
  if (lds > SLODE_FORECAST_SUMMARY_LDS_MAX) return hipErrorInvalidValue;
  FsK k{};
  fwd_fill(k.d, d);
  k.d.f.T = a.T_out;
  k.mean = a.mean; k.sd = a.sd; k.has_thr = a.has_thr; k.sense = a.sense; k.W = a.window; k.i0 = a.first_point;
  for (int c = 0; c < SLODE_MAX_C; ++c) k.thr[c] = a.thr[c];
  k.o = fs_lds(s, a.window, fwd_generic(s, d.force_generic));
  fwd_dispatch(s, d.force_generic, [&](auto sc) { fwd_launch("forecast_summary", forecast_summary_kernel<decltype(sc)::value>, d.grid, lds, stream, k); });
  return hipGetLastError();
}
