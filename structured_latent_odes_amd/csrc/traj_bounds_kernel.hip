// Per-trajectory bounds from K latent draws (slode_traj_bounds): for every trajectory b the K per-draw losses
//   loss[k][b] = -(log-likelihood + log p(z | labels) - log q(z | x)) (+ proc's 46 x label terms),  z = loc(x_b) + scale(x_b) eps[k][b]
// -- the main loss of the single row b on draw k -- kept apart, and their four summaries: the mean (-ELBO of the trajectory), the
// importance-weighted bound -log(1/K sum_k exp(-loss)), the effective sample size of the weights, the mean negative log-likelihood.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. K - 1:
// The forward phases B0 (weights), B3-B5 (fwd_solve), the state and head values of B6, the prior nets of B1 and the logits of B7 are the
// shared ones of slode_forward.h; B1 / B2 are this kernel's own: it keeps both distributions for the KL terms.
//   B0  once per workgroup: the weights every draw reuses (fwd_stage_weights: [w_t | u_j | W_g | W_d] per hidden unit, the
//       z-columns of the hidden layer and the init net, the init net's output layer, the head weights, the biases) and the likelihood
//       scale table of the fold launch (1 / scale and log scale per (c, t)) into the LDS
//   B1  once per trajectory: labels; loc / scale of the posterior (encoder launch) and the conditional prior nets, kept in the registers
//       of thread l; the observation row into the LDS as [C][T] -- HBM is read once per trajectory, not once per draw
//   per draw:
//   B2  z = loc + scale * eps_k (row b of drawing call n + k, or of the explicit [K, B, L] tensor); log q - log p of thread l
//   B3-B5  fwd_solve over the whole grid: the init net and x0, the step table, the forward affine scan
//   B6  thread <-> time point: decoder heads + ALD / Gaussian log-likelihood against the staged observations
//   B7  proc family: the main loss's label terms on z, a half-wave per label head (as phase E5 of eval_stats_kernel, use 2)
//   B8  fixed-order sums over the workgroup of (log q - log p) and of the log-likelihood; thread 0 forms loss[k] and its likelihood part
//   B9  once per trajectory, over the K stored values, in fp64: min, sums, sum exp, sum exp^2 -> the four slots as ONE 16-byte store;
//       loss_kb with plain per-lane stores
// Every sum runs in a fixed order that depends on (K, T, L) alone: the result is a function of (parameters, inputs, noise) -- bitwise equal
// between runs, between one workgroup per trajectory and the persistent loop, between in-kernel and explicit noise.  No atomics.
#include "slode_forward.h"

namespace {

constexpr int TB_NT = FWD_NT;
constexpr float TB_HL2PI = FWD_HL2PI;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct TbLds { FwdLds f; int obs, inv, lg, item, red, dred, loss, nll, total; };

struct TbK {
  FwdK f;
  PriorK pr;
  LabelHeadK lh;
  int gauss, nd, t_major;
  float tau[3];
  const float* obs;
  long long sb;
  const float *loc, *scale, *eps, *u, *sigtab;
  float *bounds, *loss_kb;
  TbLds o;
  RngK rng;
  LabelSrc lab;
};

// sum over the wave of a double, the same bits in every lane (xor butterfly: both partners add the same two values)
__device__ __forceinline__ double tb_wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// B9: the K stored losses of one trajectory -> its four slots, in fp64; thread i takes draws i, i + 256, ... in that order, then a fixed
// tree over the lanes and the waves.  Not inlined: the fp64 exp / log constants would otherwise be hoisted out of the draw loop and stay
// live in registers through every phase of the kernel (30 VGPRs more in every instantiation).
__device__ __noinline__ void tb_reduce_draws(const float* s_loss, const float* s_nll, double* s_dred, int nd, int B, int b,
                                             float* __restrict__ bounds, float* __restrict__ loss_kb) {
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
    *reinterpret_cast<f4_t*>(bounds + (long long)b * SLODE_BOUND_SLOTS) = o;   // the row's four slots: one 16-byte store
  }
  if (loss_kb)
    for (int q = tid; q < nd; q += TB_NT) loss_kb[(long long)q * B + b] = s_loss[q];
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
// LAB: the main loss scores the labels (aux_in_main: proc) -- phase B7 exists; without it the label-head code costs no registers
template <int SC, bool LAB>
__global__ void __launch_bounds__(TB_NT) traj_bounds_kernel(const TbK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_tb[];
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = tid >> 5, j32 = tid & 31;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, Q = f.Q, CT = C * T, nd = k.nd;
  const FwdSm sm = fwd_sm(s_tb, k.o.f);
  float* s_obs = s_tb + k.o.obs;   // [C][T] the trajectory's observations
  float* s_inv = s_tb + k.o.inv;   // [C][T] 1 / likelihood scale
  float* s_lg = s_tb + k.o.lg;     // [C][T] log(scale) (Gauss) or log(2 scale) (ALD)
  float* s_item = s_tb + k.o.item; // [n_aux] -46 x label log-prob of the draw, per head
  float* s_red = s_tb + k.o.red;   // [2][4] per-wave sums of (log q - log p) and of the log-likelihood
  float* s_loss = s_tb + k.o.loss; // [K] the trajectory's per-draw losses
  float* s_nll = s_tb + k.o.nll;   // [K] their negative log-likelihood parts
  double* s_dred = reinterpret_cast<double*>(s_tb + k.o.dred);   // [3][4] per-wave fp64 partials of B9 | [1] the minimum (as a double)
  const int n_items = LAB ? k.lh.n_aux : 0;

  // ---- B0: the weights every draw reuses; the likelihood scale table ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  for (int i = tid; i < CT; i += TB_NT) { s_inv[i] = k.sigtab[CT + i]; s_lg[i] = k.sigtab[2 * CT + i]; }

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- B1 ----
    __syncthreads();   // (B0's writes; the previous trajectory's readers of s_u / s_obs / s_loss / s_nll are done)
    if (tid < k.pr.nu) sm.u[tid] = slode_label_at(k.lab, k.u, k.pr.nu, b, tid);
    {   // the dense block of C*T observations in memory order (coalesced), into [C][T]
      const float* ob = k.obs + (long long)b * k.sb;
      for (int i = tid; i < CT; i += TB_NT) {
        int c, t;
        if (k.t_major) { t = i / C; c = i - t * C; } else { c = i / T; t = i - c * T; }
        s_obs[c * T + t] = ob[i];
      }
    }
    __syncthreads();
    float loc = 0.f, sc = 1.f, pl = 0.f, pls = 0.f, ips = 1.f, nlsc = 0.f;   // thread l < L keeps its latent dim's posterior and prior
    if (tid < L) {
      const int l = tid;
      loc = k.loc[(long long)b * L + l]; sc = k.scale[(long long)b * L + l];
      fwd_prior_at(k.pr, par, sm.u, l, pl, pls);
      ips = expf(-pls); nlsc = -logf(sc);
    }
    for (int kk = 0; kk < nd; ++kk) {
      // ---- B2: draw kk = row b of drawing call n + kk; log q - log p ----
      float klt = 0.f;
      if (tid < L) {
        const float z = fmaf(sc, slode_eps_at(k.rng, k.eps, b, L, tid, kk, f.B), loc);
        const float dz = (z - pl) * ips, zq = (z - loc) / sc;
        klt = (nlsc - TB_HL2PI - 0.5f * zq * zq) - (-pls - TB_HL2PI - 0.5f * dz * dz);
        sm.z[tid] = z;
      }
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] / s_item / s_red are done)
      fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // B3 - B5
      // ---- B6: heads + log-likelihood of the thread's time points ----
      float llt = 0.f;
      for (int t = tid; t < T; t += TB_NT) {
        float x[SM];
        fwd_state_at<SM>(sm, S, t, x);
        float ll = 0.f;
        for (int c = 0; c < C; ++c) {
          const float obv = s_obs[c * T + t], inv = s_inv[c * T + t], lg = s_lg[c * T + t];
          for (int q = 0; q < Q; ++q) {
            const float mu = fwd_head_value<SM>(sm, S, q * C + c, x), r = obv - mu;
            if (k.gauss) ll += -lg - TB_HL2PI - 0.5f * r * r * inv * inv;
            else ll += ((obv >= mu) ? k.tau[q] : 1.f - k.tau[q]) * (-lg - fabsf(r) * inv);
          }
        }
        llt += ll;
      }
      // ---- B7: the main loss's label terms on z (proc); half-wave = head, lane = hidden unit ----
      if (LAB) {   // (every lane of a wave takes part in every sum)
        const bool on = hw < n_items;
        const int a = on ? hw : 0;
        const slode_aux ax = k.lh.aux[a];
        const int ud = ax.u_dim;
        float lg[8];
        fwd_label_logits(k.lh, par, a, sm.z + ax.z_off, j32, lg);
        float lp = 0.f;
        if (ax.kind == SLODE_AUX_SOFTMAX) {
          float mx = -3.0e38f, se = 0.f;
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) mx = fmaxf(mx, lg[q]);
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) se += expf(lg[q] - mx);
          const float lse = mx + logf(se);
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) lp = fmaf(sm.u[ax.u_off + q], lg[q] - lse, lp);
        } else if (ax.kind == SLODE_AUX_SIGMOID) {
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) {
            const float o = lg[q], y = sm.u[ax.u_off + q];
            const float sp_pos = (o > 0.f ? o : 0.f) + log1pf(expf(-fabsf(o)));
            lp += y * (o - sp_pos) + (1.f - y) * (-sp_pos);
          }
        } else {   // EXPEXP: Laplace(exp(head 0), softplus(constant_std_*))
          const float bsc = softplusf(par[k.lh.aux_c[a]]), ib = 1.f / bsc;
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) {
            const float lc = expf(lg[q]), y = sm.u[ax.u_off + q];
            lp += -logf(2.f * bsc) - fabsf(y - lc) * ib;
          }
        }
        if (on && j32 == 0) s_item[a] = -k.lh.aux_mult * lp;
      }
      // ---- B8: fixed-order sums over the workgroup; the draw's loss ----
      klt = wave_sum(klt);
      llt = wave_sum(llt);
      if (lane == 0) { s_red[wave] = klt; s_red[4 + wave] = llt; }
      __syncthreads();
      if (tid == 0) {
        const float kl = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]), ll = (s_red[4] + s_red[5]) + (s_red[6] + s_red[7]);
        float loss = kl - ll;
        for (int a = 0; a < n_items; ++a) loss += s_item[a];
        s_loss[kk] = loss; s_nll[kk] = -ll;
      }
    }
    // ---- B9: the K stored values -> the four slots and loss_kb ----
    __syncthreads();
    tb_reduce_draws(s_loss, s_nll, s_dred, nd, f.B, b, k.bounds, k.loss_kb);
  }
}

TbLds tb_lds(const slode_shape& s, int nd, bool generic) {
  const int CT = s.C * s.T;
  LdsCarve cv;
  TbLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.obs = cv.take(CT); o.inv = cv.take(CT); o.lg = cv.take(CT); o.item = cv.take(SLODE_MAX_AUX); o.red = cv.take(8);
  o.dred = cv.take(24);   // 12 doubles (the offset is a multiple of 4 floats: 16-byte aligned)
  // the K losses and their likelihood parts come last; a K that cannot fit anyway counts as the whole budget (no overflow of the offsets)
  const int kd = nd < SLODE_TRAJ_BOUNDS_LDS_MAX / 4 ? nd : SLODE_TRAJ_BOUNDS_LDS_MAX / 4;
  o.loss = cv.take(kd); o.nll = cv.take(kd);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_traj_bounds_lds_bytes(const slode_shape& s, int num_draws, int force_generic) {
  return (size_t)tb_lds(s, num_draws, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_traj_bounds(const TrajBoundsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  TbK k{};
  fwd_fill(k.f, s, lay, a.params, a.times, a.stage_t); fwd_fill(k.pr, s, lay); fwd_fill(k.lh, s, lay);
  k.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; k.nd = a.num_draws; k.t_major = a.t_major;
  k.tau[0] = 0.5f; k.tau[1] = 0.5f + s.quantile_diff; k.tau[2] = 0.5f - s.quantile_diff;
  k.obs = a.obs; k.sb = a.sb;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u; k.sigtab = a.sigtab; k.bounds = a.bounds; k.loss_kb = a.loss_kb;
  k.rng = a.rng; k.lab = a.lab; k.o = tb_lds(s, a.num_draws, fwd_generic(s, a.force_generic));
  const size_t lds = slode_traj_bounds_lds_bytes(s, a.num_draws, a.force_generic);
  if (lds > SLODE_TRAJ_BOUNDS_LDS_MAX || a.num_draws < 1 || a.grid < 1 || s.n_aux > SLODE_MAX_AUX) return hipErrorInvalidValue;
  const bool lab = s.aux_in_main && s.n_aux > 0;
  fwd_dispatch(s, a.force_generic, [&](auto sc) {
    constexpr int SC = decltype(sc)::value;
    if (lab) fwd_launch("traj_bounds", traj_bounds_kernel<SC, true>, a.grid, lds, stream, k);
    else fwd_launch("traj_bounds", traj_bounds_kernel<SC, false>, a.grid, lds, stream, k);
  });
  return hipGetLastError();
}
