// The arithmetic of the fold W_eff[m][kappa(c, t)] = sum_f sum_j lin.weight[m][f][t - j] * w'[f][c][j] (encoder_fused.hip), written once
// in two shapes: one output per quad of lanes (fold_out_partial: the in-launch fold of enc_chain_kernel) and FW consecutive time points
// per quad from one register window of taps (fold_window_partial: weff_kernel).  Both run the same operations in the same order on every
// output -- the quad lane fh owns the filters [fh * fper, (fh + 1) * fper) in ascending order; per filter the taps j ascend, even j into
// acc0 and odd j into acc1; a tap index outside [0, n_pool) enters its multiply-add as zero (read clamped and replaced by zero, or read
// from the zeros of a padded copy of the row); the lane's value is acc0 + acc1; the quad's four values meet as (p0 + p1) + (p2 + p3) --
// hence the same bits.  Everything is host- and device-callable and needs no other header,
// so that tests/fold_math/fold_math.cpp holds the two shapes equal bit for bit and to an fp64 sum without a device
// (tests/test_fold_math_cpu.py).
#pragma once

constexpr int FOLD_WFG = 4;   // lanes per output (filter groups): one quad
// the filters whose reads the windowed shape issues together: every filter a lane can own (SLODE_MAX_F / FOLD_WFG = 4) while the windows
// fit the registers (JM <= 14: every reference config), two in the long-tap form
__host__ __device__ constexpr int fold_window_batch(int JM) { return JM <= 14 ? 4 : 2; }

__host__ __device__ __forceinline__ int fold_clamp(int i, int hi) { return i < 0 ? 0 : (i > hi ? hi : i); }
// the filters of quad lane fh: [f0, f1)
__host__ __device__ __forceinline__ void fold_filters(int F, int fh, int& f0, int& f1) {
  const int fper = (F + FOLD_WFG - 1) / FOLD_WFG;
  f0 = fh * fper;
  f1 = (fh + 1) * fper < F ? (fh + 1) * fper : F;
}

// Lane fh's share of ONE output W_eff[m][kappa(c, t)].  wlm: row m of lin.weight [F][n_pool]; wp: w' [F][C][JM] (zero beyond J).
template <int JM>
__host__ __device__ __forceinline__ float fold_out_partial(int F, int C, int n_pool, const float* __restrict__ wlm, const float* __restrict__ s_wp,
                                                           int c, int t, int fh) {
  int f0, f1;
  fold_filters(F, fh, f0, f1);
  float acc0 = 0.f, acc1 = 0.f;
#pragma unroll 2
  for (int f = f0; f < f1; ++f) {
    const float* wl = wlm + f * n_pool;
    const float* wp = s_wp + (f * C + c) * JM;
    float v[JM];
#pragma unroll
    for (int j = 0; j < JM; ++j) v[j] = wl[fold_clamp(t - j, n_pool - 1)];   // unconditional, clamped
#pragma unroll
    for (int j = 0; j < JM; j += 2) {
      acc0 = fmaf((t - j >= 0 && t - j < n_pool) ? v[j] : 0.f, wp[j], acc0);
      if (j + 1 < JM) acc1 = fmaf((t - j - 1 >= 0 && t - j - 1 < n_pool) ? v[j + 1] : 0.f, wp[j + 1], acc1);
    }
  }
  return acc0 + acc1;
}

// Lane fh's share of the FW outputs t0 .. t0 + FW - 1 of one (m, c).  Per filter the FW + JM - 1 taps lin[m][f][t0 - (JM - 1) .. t0 + FW - 1]
// are read once (the output t0 + w takes its tap j from window slot w - j + JM - 1) and the JM values of w'[f][c][.] once; the clamp and the
// select-zero of a tap depend on its index alone, so they are done once per slot.  NB filters' reads are issued before the first
// multiply-add of the batch (NB >= the lane's filter count: all of them, one wait).  Time points at or beyond T are computed from
// in-bounds reads and are the caller's to drop.
// PADDED: the caller's copy of the row holds zeros around every filter's n_pool values (fold_pad / fold_padded_at below; stride: the
// distance between two filters' values, n_pool + fold_pad) -- a tap index outside [0, n_pool) then READS the zero that the select would
// put in its place: the multiply-add sees the same operands, and a tap costs one read at a constant offset, no index arithmetic.
// Not PADDED (stride = n_pool): clamped index, select-zero.
template <int JM, int FW, int NB, bool PADDED>
__host__ __device__ __forceinline__ void fold_window_partial(int F, int C, int n_pool, int stride, const float* __restrict__ wlm,
                                                             const float* __restrict__ s_wp, int c, int t0, int fh, float (&r)[FW]) {
  constexpr int NV = FW + JM - 1;
  int f0, f1;
  fold_filters(F, fh, f0, f1);
  float acc0[FW], acc1[FW];
#pragma unroll
  for (int w = 0; w < FW; ++w) acc0[w] = acc1[w] = 0.f;
  for (int fb = f0; fb < f1; fb += NB) {
    float v[NB][NV], p[NB][JM];
#pragma unroll
    for (int q = 0; q < NB; ++q)
      if (fb + q < f1) {
        const float* wl = wlm + (fb + q) * stride;
        const float* wp = s_wp + ((fb + q) * C + c) * JM;
#pragma unroll
        for (int i = 0; i < NV; ++i) v[q][i] = PADDED ? wl[t0 - (JM - 1) + i] : wl[fold_clamp(t0 - (JM - 1) + i, n_pool - 1)];   // unconditional
#pragma unroll
        for (int j = 0; j < JM; ++j) p[q][j] = wp[j];
      }
#pragma unroll
    for (int q = 0; q < NB; ++q)
      if (fb + q < f1) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
          const int idx = t0 - (JM - 1) + i;
          if (!PADDED) v[q][i] = (idx >= 0 && idx < n_pool) ? v[q][i] : 0.f;
        }
#pragma unroll
        for (int w = 0; w < FW; ++w)
#pragma unroll
          for (int j = 0; j < JM; j += 2) {
            acc0[w] = fmaf(v[q][w - j + JM - 1], p[q][j], acc0[w]);
            if (j + 1 < JM) acc1[w] = fmaf(v[q][w - j - 1 + JM - 1], p[q][j + 1], acc1[w]);
          }
      }
  }
#pragma unroll
  for (int w = 0; w < FW; ++w) r[w] = acc0[w] + acc1[w];
}

// The padded copy of n_rows * F filter rows: fold_pad zeros, then per filter row its n_pool values and fold_pad zeros -- a window reaches
// at most JM - 1 below index 0 and J - 1 + FW - 1 <= fold_pad beyond n_pool - 1 (t0 + FW - 1 <= T - 1 + FW - 1 = n_pool + J - 2 + FW - 1).
__host__ __device__ constexpr int fold_pad(int JM, int FW) { return JM - 1 + FW - 1; }
__host__ __device__ __forceinline__ int fold_padded_size(int n_rows, int F, int n_pool, int pad) { return n_rows * F * (n_pool + pad) + pad; }
// where value q of filter row fr (counted over all the rows of the copy) lies; the zeros: [fr * (n_pool + pad), + pad) for fr = 0 .. n_rows * F
__host__ __device__ __forceinline__ int fold_padded_at(int fr, int q, int n_pool, int pad) { return pad + fr * (n_pool + pad) + q; }

// What the two quad DPP adds of the device leave in every lane of the quad (r += r[lane ^ 1]; r += r[lane ^ 2]), for the host.
__host__ __device__ __forceinline__ float fold_quad_sum(const float (&p)[FOLD_WFG]) { return (p[0] + p[1]) + (p[2] + p[3]); }

// The work items of the windowed fold: one quad per (m, c, window of FW time points), a row of W_eff being C * ceil(T / FW) consecutive
// items ordered as its memory is -- kappa = t * C + c: (window, c); kappa = c * T + t: (c, window).
__host__ __device__ __forceinline__ int fold_windows(int T, int FW) { return (T + FW - 1) / FW; }
__host__ __device__ __forceinline__ void fold_item(int it, int T, int C, int t_major, int FW, int& m, int& c, int& t0) {
  const int nwin = fold_windows(T, FW), per = C * nwin;
  m = it / per;
  const int rem = it - m * per;
  int win;
  if (t_major) { win = rem / C; c = rem - win * C; } else { c = rem / nwin; win = rem - c * nwin; }
  t0 = win * FW;
}
__host__ __device__ __forceinline__ int fold_kappa(int T, int C, int t_major, int c, int t) { return t_major ? t * C + c : c * T + t; }
