// The per-draw routines of the kernels that score the K latent draws of a trajectory (traj_bounds_kernel and label_evidence_kernel in
// traj_bounds_kernel.hip, pointwise_kernel.hip): log q - log p of a latent dim, the log-likelihood of a thread's time points, the label
// log-probability of a head, and the fp64 reduction of the K stored losses.  Every kernel executes the same routines: equal inputs give
// equal bits.
#pragma once
#include "slode_forward.h"

namespace {

constexpr int TB_NT = FWD_NT;
constexpr float TB_HL2PI = FWD_HL2PI;

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

// ---- the per-draw terms traj_bounds_kernel and label_evidence_kernel both execute (the same routines: column v of the evidence is bit for
// bit the bounds of that label set) ----
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

}  // namespace
