// What the kernels that score the K latent draws of a trajectory share (traj_bounds_kernel and label_evidence_kernel in traj_bounds_kernel.hip,
// pointwise_kernel.hip, pointwise_loo_kernel.hip, refine_kernel.hip), each piece ONCE: the kernel-argument part ScoredK and its fill from ScoredLaunch, the
// LDS pieces of the frame (scored_lds / scored_sm), the staging of the scale table and of a trajectory's observations (and mask), the
// posterior and prior of a latent dim, and the per-draw routines: log q - log p of a latent dim, the log-likelihood of a thread's time
// points (plain and weighted), the label log-probability of a head, the workgroup sums that form a draw's loss, the whole draw loop of
// traj_bounds_kernel and of pointwise_kernel's importance sweep, and the fp64 reduction of the K stored losses.  Every kernel executes the
// same routines: equal inputs give equal bits.
#pragma once
#include "slode_forward.h"

namespace {

constexpr int TB_NT = FWD_NT;
constexpr float TB_HL2PI = FWD_HL2PI;

// ---- the frame: kernel arguments, LDS pieces, staging ------------------------------------------------------------------------------
// the kernel-argument part (after FwdK f, PriorK pr and, where the kernel scores labels, LabelHeadK lh); mask: nullptr = all 1
struct ScoredK {
  int gauss, nd, t_major;
  float tau[3];
  const float *obs, *mask;
  long long sb;
  const float *loc, *scale, *eps, *u, *sigtab;
  RngK rng;
  LabelSrc lab;
};
inline void fwd_fill(ScoredK& k, const ScoredLaunch& a) {
  const slode_shape& s = a.s;
  k.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; k.nd = a.num_draws; k.t_major = a.t_major;
  k.tau[0] = 0.5f; k.tau[1] = 0.5f + s.quantile_diff; k.tau[2] = 0.5f - s.quantile_diff;
  k.obs = a.obs; k.mask = a.mask; k.sb = a.sb;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u; k.sigtab = a.sigtab;
  k.rng = a.rng; k.lab = a.lab;
}

// offsets (in floats, multiples of 4) of the frame's LDS pieces, carved right after fwd_lds; a piece of 0 floats: the kernel has none
struct ScoredLds { int obs, inv, lg, w, item, red, dred; };
inline ScoredLds scored_lds(LdsCarve& cv, const slode_shape& s, bool masked, int n_item, int n_dred) {
  const int CT = s.C * s.T;
  ScoredLds o{};
  o.obs = cv.take(CT); o.inv = cv.take(CT); o.lg = cv.take(CT); o.w = cv.take(masked ? CT : 0); o.item = cv.take(n_item); o.red = cv.take(8);
  o.dred = cv.take(n_dred);   // tb_reduce_draws: 24 floats = 12 doubles (the offset is a multiple of 4 floats: 16-byte aligned)
  return o;
}
struct ScoredSm {
  float *obs, *inv, *lg;   // [C][T] the trajectory's observations | 1 / likelihood scale | log(scale) (Gauss) or log(2 scale) (ALD)
  float* w;                // [C][T] the weights of the likelihood terms (the masked kernels)
  float* item;             // [n_aux] -46 x label log-prob of the draw, per head
  float* red;              // [2][4] per-wave sums of (log q - log p) and of the log-likelihood
  double* dred;            // [3][4] per-wave fp64 partials of tb_reduce_draws
};
__device__ __forceinline__ ScoredSm scored_sm(float* base, const ScoredLds& o) {
  return ScoredSm{base + o.obs, base + o.inv, base + o.lg, base + o.w, base + o.item, base + o.red, reinterpret_cast<double*>(base + o.dred)};
}

// B0, second line: the likelihood scale table of the fold launch (1 / scale and log scale per (c, t)) into the LDS
__device__ __forceinline__ void tb_stage_scales(const ScoredK& d, const ScoredSm& sc, int CT, int tid) {
  for (int i = tid; i < CT; i += TB_NT) { sc.inv[i] = d.sigtab[CT + i]; sc.lg[i] = d.sigtab[2 * CT + i]; }
}
// B1: the dense block of C*T observations of trajectory b (MASKED: and its weights; no mask: all 1) in memory order (coalesced), into [C][T]
template <bool MASKED>
__device__ __forceinline__ void tb_stage_obs(const ScoredK& d, const ScoredSm& sc, long long b, int T, int C, int tid) {
  const float* ob = d.obs + b * d.sb;
  const float* mk = MASKED && d.mask ? d.mask + b * d.sb : nullptr;
  for (int i = tid; i < C * T; i += TB_NT) {
    int c, t;
    if (d.t_major) { t = i / C; c = i - t * C; } else { c = i / T; t = i - c * T; }
    sc.obs[c * T + t] = ob[i];
    if (MASKED) sc.w[c * T + t] = mk ? mk[i] : 1.f;
  }
}
// B1's tail: thread l < L keeps its latent dim's posterior (loc, sc, nlsc = -log sc) and, with prior, its conditional prior on the staged
// labels s_u (pl, pls, ips = exp(-pls))
struct TbDim { float loc = 0.f, sc = 1.f, nlsc = 0.f, pl = 0.f, pls = 0.f, ips = 1.f; };
__device__ __forceinline__ void tb_dim_load(TbDim& q, const ScoredK& d, const PriorK& pr, const float* __restrict__ par, const float* s_u,
                                            long long b, int L, int l, bool prior) {
  q.loc = d.loc[b * L + l]; q.sc = d.scale[b * L + l];
  if (prior) { fwd_prior_at(pr, par, s_u, l, q.pl, q.pls); q.ips = expf(-q.pls); q.nlsc = -logf(q.sc); }
}

// sum over the wave of a double, the same bits in every lane (xor butterfly: both partners add the same two values)
__device__ __forceinline__ double tb_wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// B9: the K stored losses of one trajectory -> its four slots, in fp64; thread i takes draws i, i + 256, ... in that order, then a fixed
// tree over the lanes and the waves.  Not inlined: the fp64 exp / log constants would otherwise be hoisted out of the draw loop and stay
// live in registers through every phase of the kernel (30 VGPRs more in every instantiation).  row: the four slots' destination (global
// memory for traj_bounds, the LDS for label_evidence, which replaces slot 3 before its own store); bound64 (or nullptr): slot 1 before it
// is rounded.  A barrier must separate two calls (the second call's first partials overwrite what thread 0 of the first still reads).
__device__ __noinline__ void tb_reduce_draws(const float* s_loss, const float* s_nll, double* s_dred, int nd, int B, int b,
                                             float* row, float* __restrict__ loss_kb, double* bound64) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double sl = 0.0, sn = 0.0;
  float mn = 3.4028234664e38f;
  for (int q = tid; q < nd; q += TB_NT) { const float v = s_loss[q]; sl += (double)v; sn += (double)s_nll[q]; mn = fminf(mn, v); }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off, 64));
  sl = tb_wave_sum_d(sl); sn = tb_wave_sum_d(sn);
  if (lane == 0) { s_dred[wave] = sl; s_dred[4 + wave] = sn; s_dred[8 + wave] = (double)mn; }
  __syncthreads();
  const double mnd = fmin(fmin(s_dred[8], s_dred[9]), fmin(s_dred[10], s_dred[11]));
  sl = (s_dred[0] + s_dred[1]) + (s_dred[2] + s_dred[3]);
  sn = (s_dred[4] + s_dred[5]) + (s_dred[6] + s_dred[7]);
  double sw = 0.0, sw2 = 0.0;   // w_k = exp(min - loss_k) in (0, 1], the minimum's weight exactly 1
  for (int q = tid; q < nd; q += TB_NT) { const double w = exp(mnd - (double)s_loss[q]); sw += w; sw2 = fma(w, w, sw2); }
  sw = tb_wave_sum_d(sw); sw2 = tb_wave_sum_d(sw2);
  __syncthreads();   // (every thread has read the first pass's partials)
  if (lane == 0) { s_dred[wave] = sw; s_dred[4 + wave] = sw2; }
  __syncthreads();
  if (tid == 0) {
    typedef float f4_t __attribute__((ext_vector_type(4)));
    sw = (s_dred[0] + s_dred[1]) + (s_dred[2] + s_dred[3]);
    sw2 = (s_dred[4] + s_dred[5]) + (s_dred[6] + s_dred[7]);
    const double dk = (double)nd;
    f4_t o;
    o.x = (float)(sl / dk);
    o.y = (float)(mnd - log(sw / dk));
    o.z = (float)(sw * sw / sw2);
    o.w = (float)(sn / dk);
    *reinterpret_cast<f4_t*>(row) = o;   // the row's four slots: one 16-byte store
    if (bound64) *bound64 = mnd - log(sw / dk);
  }
  if (loss_kb)
    for (int q = tid; q < nd; q += TB_NT) loss_kb[(long long)q * B + b] = s_loss[q];
}

// ---- the per-draw terms (the same routines in every kernel: column v of the evidence is bit for bit the bounds of that label set, refine
// at J = 0 and pointwise's importance sweep give the losses of traj_bounds) ----
// B2: log q(z | x) - log p(z | labels) of one latent dim: posterior loc / sc / nlsc = -log sc, prior pl / pls and ips = exp(-pls)
__device__ __forceinline__ float tb_logq_minus_logp(float z, float loc, float sc, float nlsc, float pl, float pls, float ips) {
  const float dz = (z - pl) * ips, zq = (z - loc) / sc;
  return (nlsc - TB_HL2PI - 0.5f * zq * zq) - (-pls - TB_HL2PI - 0.5f * dz * dz);
}

// B6: decoder heads + ALD / Gaussian log-likelihood of the thread's time points tid, tid + 256, ... against the staged observations
template <int SM>
__device__ __forceinline__ float tb_loglik_points(const FwdSm& sm, int S, int T, int C, int Q, int gauss, const float (&tau)[3],
                                                  const float* s_obs, const float* s_inv, const float* s_lg, int tid) {
  float llt = 0.f;
  for (int t = tid; t < T; t += TB_NT) {
    float x[SM];
    fwd_state_at<SM>(sm, S, t, x);
    float ll = 0.f;
    for (int c = 0; c < C; ++c) {
      const float obv = s_obs[c * T + t], inv = s_inv[c * T + t], lg = s_lg[c * T + t];
      for (int q = 0; q < Q; ++q) {
        const float mu = fwd_head_value<SM>(sm, S, q * C + c, x), r = obv - mu;
        if (gauss) ll += -lg - TB_HL2PI - 0.5f * r * r * inv * inv;
        else ll += ((obv >= mu) ? tau[q] : 1.f - tau[q]) * (-lg - fabsf(r) * inv);
      }
    }
    llt += ll;
  }
  return llt;
}

// B6 of ONE point: l[i] of point i = (c, t), the addends of tb_loglik_points for channel c summed over the Q heads, from the state x at t
// (pointwise_kernel's and pointwise_loo_kernel's point folds: the same routine, the same bits)
template <int SM>
__device__ __forceinline__ float tb_point_loglik(const FwdSm& sm, int S, int C, int Q, int c, int gauss, const float (&tau)[3], float obv, float inv,
                                                 float lg, const float (&x)[SM]) {
  float l = 0.f;
  for (int q = 0; q < Q; ++q) {
    const float mu = fwd_head_value<SM>(sm, S, q * C + c, x), r = obv - mu;
    if (gauss) l += -lg - TB_HL2PI - 0.5f * r * r * inv * inv;
    else l += ((obv >= mu) ? tau[q] : 1.f - tau[q]) * (-lg - fabsf(r) * inv);
  }
  return l;
}

// B7: the log-probability of the label columns y[0 .. u_dim) of head a under its logits lg (no cross-lane operation)
__device__ __forceinline__ float tb_label_logprob(const LabelHeadK& lh, const float* __restrict__ par, int a, const float (&lg)[8], const float* y) {
  const slode_aux ax = lh.aux[a];
  const int ud = ax.u_dim;
  float lp = 0.f;
  if (ax.kind == SLODE_AUX_SOFTMAX) {
    float mx = -3.0e38f, se = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q < ud) mx = fmaxf(mx, lg[q]);
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q < ud) se += expf(lg[q] - mx);
    const float lse = mx + logf(se);
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q < ud) lp = fmaf(y[q], lg[q] - lse, lp);
  } else if (ax.kind == SLODE_AUX_SIGMOID) {
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q < ud) {
      const float o = lg[q], yy = y[q];
      const float sp_pos = (o > 0.f ? o : 0.f) + log1pf(expf(-fabsf(o)));
      lp += yy * (o - sp_pos) + (1.f - yy) * (-sp_pos);
    }
  } else {   // EXPEXP: Laplace(exp(head 0), softplus(constant_std_*))
    const float bsc = softplusf(par[lh.aux_c[a]]), ib = 1.f / bsc;
#pragma unroll
    for (int q = 0; q < 8; ++q) if (q < ud) {
      const float lc = expf(lg[q]), yy = y[q];
      lp += -logf(2.f * bsc) - fabsf(yy - lc) * ib;
    }
  }
  return lp;
}

// B6 with a weight on every term (refine_kernel's R4, pointwise_kernel's P6: at w = 1 the sum of tb_loglik_points); GRAD && bwd: also
// g_x[t][s] = -sum_{c,q} w dll/dmu hw[qc][s] of those points into s_g [T][S]
template <int SM, bool GRAD>
__device__ __forceinline__ float tb_loglik_weighted(const FwdSm& sm, int S, int T, int C, int Q, int gauss, const float (&tau)[3], const ScoredSm& sc,
                                                    bool bwd, float* s_g, int tid) {
  float llt = 0.f;
  for (int t = tid; t < T; t += TB_NT) {
    float x[SM], gx[SM];
    fwd_state_at<SM>(sm, S, t, x);
#pragma unroll
    for (int s = 0; s < SM; ++s) gx[s] = 0.f;
    float ll = 0.f;
    for (int c = 0; c < C; ++c) {
      const float obv = sc.obs[c * T + t], inv = sc.inv[c * T + t], lg = sc.lg[c * T + t], w = sc.w[c * T + t];
      for (int q = 0; q < Q; ++q) {
        const float mu = fwd_head_value<SM>(sm, S, q * C + c, x), r = obv - mu;
        float gmu;   // w dll / dmu
        if (gauss) {
          ll += w * (-lg - TB_HL2PI - 0.5f * r * r * inv * inv);
          gmu = w * (r * inv * inv);
        } else {
          const float wq = (obv >= mu) ? tau[q] : 1.f - tau[q];
          ll += (w * wq) * (-lg - fabsf(r) * inv);
          gmu = w * (inv * ((obv >= mu) ? tau[q] : -(1.f - tau[q])));
        }
        if (GRAD && bwd) {
#pragma unroll
          for (int s = 0; s < SM; ++s) if (s < S) gx[s] = fmaf(-gmu, sm.hw[(q * C + c) * S + s], gx[s]);
        }
      }
    }
    if (GRAD && bwd) {
#pragma unroll
      for (int s = 0; s < SM; ++s) if (s < S) s_g[t * S + s] = gx[s];
    }
    llt += ll;
  }
  return llt;
}

// B8: fixed-order sums over the workgroup of the threads' (log q - log p) and log-likelihood; thread 0 forms the draw's loss (+ the n_items
// label terms of s_item) and, with nll, its likelihood part.  Ends after the workgroup's barrier: the caller's next barrier publishes the stores.
__device__ __forceinline__ void tb_draw_sums(float klt, float llt0, float* s_red, const float* s_item, int n_items, float* loss, float* nll) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  klt = wave_sum(klt);
  const float llt = wave_sum(llt0);
  if (lane == 0) { s_red[wave] = klt; s_red[4 + wave] = llt; }
  __syncthreads();
  if (tid == 0) {
    const float kl = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]), ll = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
    float v = kl - ll;
    for (int a = 0; a < n_items; ++a) v += s_item[a];
    *loss = v;
    if (nll) *nll = -ll;
  }
}

// B2 - B8, the draw loop of traj_bounds_kernel and of pointwise_kernel's importance sweep: the nd per-draw losses of trajectory b and their
// likelihood parts into s_loss / s_nll.  LAB: phase B7 exists (the main loss scores the labels: proc); WEIGHTED: sc.w weighs the likelihood terms.
template <int SM, bool LAB, bool WEIGHTED>
__device__ __forceinline__ void tb_draw_losses(const FwdK& f, const LabelHeadK& lh, const ScoredK& d, const FwdSm& sm, const ScoredSm& sc, int S,
                                               int b, const TbDim& q, float* s_loss, float* s_nll, int tid) {
  const float* __restrict__ par = f.params;
  const int T = f.T, L = f.L, hw = tid >> 5, j32 = tid & 31, n_items = LAB ? lh.n_aux : 0;
  for (int kk = 0; kk < d.nd; ++kk) {
    // ---- B2: draw kk = row b of drawing call n + kk; log q - log p ----
    float klt = 0.f;
    if (tid < L) {
      const float z = fmaf(q.sc, slode_eps_at(d.rng, d.eps, b, L, tid, kk, f.B), q.loc);
      klt = tb_logq_minus_logp(z, q.loc, q.sc, q.nlsc, q.pl, q.pls, q.ips);
      sm.z[tid] = z;
    }
    __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] / s_item / s_red are done)
    fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // B3 - B5
    // ---- B6: heads + log-likelihood of the thread's time points ----
    const float llt0 = WEIGHTED ? tb_loglik_weighted<SM, false>(sm, S, T, f.C, f.Q, d.gauss, d.tau, sc, false, nullptr, tid)
                                : tb_loglik_points<SM>(sm, S, T, f.C, f.Q, d.gauss, d.tau, sc.obs, sc.inv, sc.lg, tid);
    // ---- B7: the main loss's label terms on z (proc); half-wave = head, lane = hidden unit ----
    if (LAB) {   // (every lane of a wave takes part in every sum)
      const bool on = hw < n_items;
      const int a = on ? hw : 0;
      const slode_aux ax = lh.aux[a];
      float lg[8];
      fwd_label_logits(lh, par, a, sm.z + ax.z_off, j32, lg);
      const float lp = tb_label_logprob(lh, par, a, lg, sm.u + ax.u_off);
      if (on && j32 == 0) sc.item[a] = -lh.aux_mult * lp;
    }
    // ---- B8: fixed-order sums over the workgroup; the draw's loss ----
    tb_draw_sums(klt, llt0, sc.red, sc.item, n_items, s_loss + kk, s_nll + kk);
  }
}

}  // namespace
