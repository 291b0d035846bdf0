// Per-trajectory bounds from K latent draws (slode_traj_bounds): for every trajectory b the K per-draw losses
//   loss[k][b] = -(log-likelihood + log p(z | labels) - log q(z | x)) (+ proc's 46 x label terms),  z = loc(x_b) + scale(x_b) eps[k][b]
// -- the main loss of the single row b on draw k -- kept apart, and their four summaries: the mean (-ELBO of the trajectory), the
// importance-weighted bound -log(1/K sum_k exp(-loss)), the effective sample size of the weights, the mean negative log-likelihood.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. K - 1:
//   B0  once per workgroup: the weights every draw reuses (phase M0 of recon_moments_kernel: [w_t | u_j | W_g | W_d] per hidden unit, the
//       z-columns of the hidden layer and the init net, the init net's output layer, the head weights, the biases) and the likelihood
//       scale table of the fold launch (1 / scale and log scale per (c, t)) into the LDS
//   B1  once per trajectory: labels; loc / scale of the posterior (encoder launch) and the conditional prior nets, kept in the registers
//       of thread l; the observation row into the LDS as [C][T] -- HBM is read once per trajectory, not once per draw
//   per draw:
//   B2  z = loc + scale * eps_k (row b of drawing call n + k, or of the explicit [K, B, L] tensor); log q - log p of thread l
//   B3  time-invariant part of the hidden layer (into the unit's weight row) and the init net; x0
//   B4  step coefficients x' = A x + b of every grid step (tests/kernel_math.py step_coeffs), thread <-> step, all four waves
//   B5  forward affine scan: one state component per wave pass, a chunk of steps per lane, Kogge-Stone over the lanes' maps
//   B6  thread <-> time point: decoder heads + ALD / Gaussian log-likelihood against the staged observations
//   B7  proc family: the main loss's label terms on z, a half-wave per label head (phase E5 of eval_stats_kernel, use 2)
//   B8  fixed-order sums over the workgroup of (log q - log p) and of the log-likelihood; thread 0 forms loss[k] and its likelihood part
//   B9  once per trajectory, over the K stored values, in fp64: min, sums, sum exp, sum exp^2 -> the four slots as ONE 16-byte store;
//       loss_kb with plain per-lane stores
// Every sum runs in a fixed order that depends on (K, T, L) alone: the result is a function of (parameters, inputs, noise) -- bitwise equal
// between runs, between one workgroup per trajectory and the persistent loop, between in-kernel and explicit noise.  No atomics.
#include "slode_common.h"

namespace {

constexpr int TB_NT = 256;
constexpr float TB_HL2PI = 0.91893853320467274178f;
#define TB_ROW(SM) ((2 + 2 * (SM) + 3) & ~3)   // floats of one hidden unit's LDS row: w_t | u_j | W_g[0..SM) | W_d[0..SM)

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region
struct TbLds { int a, b, obs, inv, lg, row, w1, b1, w2, hw, bgd, z, u, h0, x0, item, red, loss, nll, dred, total; };

struct TbK {
  int B, T, C, L, S, H, nu, n_groups, n_aux, U, R, method, gauss, Q, nd, t_major;
  float aux_mult, tau[3];
  slode_group grp[SLODE_MAX_GROUPS];
  slode_aux aux[SLODE_MAX_AUX];
  int ploc_w[SLODE_MAX_GROUPS], ploc_b[SLODE_MAX_GROUPS], pls_w[SLODE_MAX_GROUPS], pls_b[SLODE_MAX_GROUPS];
  int init_w1, init_b1, init_w2, init_b2, dyn_wh, dyn_bh, dyn_wg, dyn_bg, dyn_wd, dyn_bd, head[SLODE_MAX_HEADS];
  int aux_w1[SLODE_MAX_AUX], aux_b1[SLODE_MAX_AUX], aux_w2[SLODE_MAX_AUX], aux_b2[SLODE_MAX_AUX], aux_c[SLODE_MAX_AUX];
  const float *params, *times, *stage_t, *obs;
  long long sb;
  const float *loc, *scale, *eps, *u, *sigtab;
  float *bounds, *loss_kb;
  TbLds o;
  RngK rng;
  LabelSrc lab;
};

// a(t, z), d(t, z) of one stage time from the LDS rows [w_t | u_j | W_g[.][j] | W_d[.][j]] (every lane reads the same address: broadcast;
// rows are 16-byte aligned: read as 16-byte LDS loads)
template <int SM>
__device__ __forceinline__ void tb_ad(const float* __restrict__ s_row, const float* __restrict__ s_bgd, int H, float t, int S,
                                      float (&a)[SM], float (&d)[SM]) {
  typedef float f4_t __attribute__((ext_vector_type(4)));
  constexpr int RW = TB_ROW(SM);
#pragma unroll
  for (int s = 0; s < SM; ++s) { a[s] = s < S ? s_bgd[s] : 0.f; d[s] = s < S ? s_bgd[S + s] : 0.f; }
  for (int j = 0; j < H; ++j) {
    float r[RW];
#pragma unroll
    for (int i = 0; i < RW / 4; ++i) {
      const f4_t v = reinterpret_cast<const f4_t*>(s_row + j * RW)[i];
      r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
    }
    const float hj = fmaxf(fmaf(r[0], t, r[1]), 0.f);
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (s < S) { a[s] = fmaf(r[2 + s], hj, a[s]); d[s] = fmaf(r[2 + SM + s], hj, d[s]); }
  }
#pragma unroll
  for (int s = 0; s < SM; ++s) { a[s] = sigmoidf_fast(a[s]); d[s] = sigmoidf_fast(d[s]); }
}

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
  const float* __restrict__ par = k.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = tid >> 5, j32 = tid & 31;
  const int T = k.T, L = k.L, S = SC ? SC : k.S, H = k.H, C = k.C, Q = k.Q, U = k.U, NS = T - 1, QC = Q * C, CT = C * T, nd = k.nd;
  constexpr int RW = TB_ROW(SM);
  float* s_A = s_tb + k.o.a;       // A[T-1][S], overwritten by x[n+1][.] in the scan
  float* s_B = s_tb + k.o.b;       // b[T-1][S]
  float* s_obs = s_tb + k.o.obs;   // [C][T] the trajectory's observations
  float* s_inv = s_tb + k.o.inv;   // [C][T] 1 / likelihood scale
  float* s_lg = s_tb + k.o.lg;     // [C][T] log(scale) (Gauss) or log(2 scale) (ALD)
  float* s_row = s_tb + k.o.row;   // [H][RW]: w_t | u_j (per draw) | W_g[0..S)[j] | W_d[0..S)[j]
  float* s_w1 = s_tb + k.o.w1;     // [L][2H]: z-columns of the hidden layer (r < H) and the init net's first layer (r >= H), transposed
  float* s_b1 = s_tb + k.o.b1;     // [2H]
  float* s_w2 = s_tb + k.o.w2;     // [H][S] init net's output layer, transposed | [S] its bias
  float* s_hw = s_tb + k.o.hw;     // [Q*C][S] head weights
  float* s_bgd = s_tb + k.o.bgd;   // [2S] growth | degradation bias
  float* s_z = s_tb + k.o.z;
  float* s_u = s_tb + k.o.u;
  float* s_h0 = s_tb + k.o.h0;
  float* s_x0 = s_tb + k.o.x0;
  float* s_item = s_tb + k.o.item; // [n_aux] -46 x label log-prob of the draw, per head
  float* s_red = s_tb + k.o.red;   // [2][4] per-wave sums of (log q - log p) and of the log-likelihood
  float* s_loss = s_tb + k.o.loss; // [K] the trajectory's per-draw losses
  float* s_nll = s_tb + k.o.nll;   // [K] their negative log-likelihood parts
  double* s_dred = reinterpret_cast<double*>(s_tb + k.o.dred);   // [3][4] per-wave fp64 partials of B9 | [1] the minimum (as a double)
  const int n_items = LAB ? k.n_aux : 0;

  // ---- B0: the weights every draw reuses; the likelihood scale table ----
  for (int i = tid; i < H * RW; i += TB_NT) {
    const int j = i / RW, c = i - j * RW;
    float v = 0.f;
    if (c == 0) v = par[k.dyn_wh + j * (1 + L)];
    else if (c >= 2 && c < 2 + S) v = par[k.dyn_wg + (c - 2) * H + j];
    else if (c >= 2 + SM && c < 2 + SM + S) v = par[k.dyn_wd + (c - 2 - SM) * H + j];
    s_row[i] = v;
  }
  for (int i = tid; i < L * 2 * H; i += TB_NT) {
    const int l = i / (2 * H), r = i - l * 2 * H;
    s_w1[i] = r < H ? par[k.dyn_wh + r * (1 + L) + 1 + l] : par[k.init_w1 + (r - H) * L + l];
  }
  for (int i = tid; i < 2 * H; i += TB_NT) s_b1[i] = i < H ? par[k.dyn_bh + i] : par[k.init_b1 + i - H];
  for (int i = tid; i < H * S + S; i += TB_NT) {
    const int j = i / S, s = i - j * S;
    s_w2[i] = i < H * S ? par[k.init_w2 + s * H + j] : par[k.init_b2 + i - H * S];
  }
  for (int i = tid; i < QC * S; i += TB_NT) {
    const int qc = i / S, q = qc / C;
    s_hw[i] = par[k.head[q] + (qc - q * C) * S + (i - qc * S)];
  }
  for (int i = tid; i < 2 * S; i += TB_NT) s_bgd[i] = i < S ? par[k.dyn_bg + i] : par[k.dyn_bd + i - S];
  for (int i = tid; i < CT; i += TB_NT) { s_inv[i] = k.sigtab[CT + i]; s_lg[i] = k.sigtab[2 * CT + i]; }

  for (int b = blockIdx.x; b < k.B; b += gridDim.x) {
    // ---- B1 ----
    __syncthreads();   // (B0's writes; the previous trajectory's readers of s_u / s_obs / s_loss / s_nll are done)
    if (tid < k.nu) s_u[tid] = slode_label_at(k.lab, k.u, k.nu, b, tid);
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
      for (int g = 0; g < k.n_groups; ++g) {
        const slode_group gr = k.grp[g];
        if (l >= gr.z_off && l < gr.z_off + gr.z_dim) {
          const int ll = l - gr.z_off;
          pl = par[k.ploc_b[g] + ll]; pls = par[k.pls_b[g] + ll];
          for (int q = 0; q < gr.u_dim; ++q) {
            const float uv = s_u[gr.u_off + q];
            pl = fmaf(par[k.ploc_w[g] + ll * gr.u_dim + q], uv, pl);
            pls = fmaf(par[k.pls_w[g] + ll * gr.u_dim + q], uv, pls);
          }
        }
      }
      ips = expf(-pls); nlsc = -logf(sc);
    }
    for (int kk = 0; kk < nd; ++kk) {
      // ---- B2: draw kk = row b of drawing call n + kk; log q - log p ----
      float klt = 0.f;
      if (tid < L) {
        const float z = fmaf(sc, slode_eps_at(k.rng, k.eps, b, L, tid, kk, k.B), loc);
        const float dz = (z - pl) * ips, zq = (z - loc) / sc;
        klt = (nlsc - TB_HL2PI - 0.5f * zq * zq) - (-pls - TB_HL2PI - 0.5f * dz * dz);
        s_z[tid] = z;
      }
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] / s_item / s_red are done)
      // ---- B3: u = W_z z + b_h into the units' rows; the init net's hidden layer ----
      if (tid < 2 * H) {
        float v = s_b1[tid];
        for (int l = 0; l < L; ++l) v = fmaf(s_w1[l * 2 * H + tid], s_z[l], v);
        if (tid < H) s_row[tid * RW + 1] = v;
        else s_h0[tid - H] = fmaxf(v, 0.f);
      }
      __syncthreads();
      if (tid < S) {
        float o = s_w2[H * S + tid];
        for (int j = 0; j < H; ++j) o = fmaf(s_w2[j * S + tid], s_h0[j], o);
        s_x0[tid] = sigmoidf_fast(o);
      }
      // ---- B4: step coefficients ----
      for (int n = tid; n < NS; n += TB_NT) {
        const float h = k.times[n + 1] - k.times[n];
        float a[SM], d[SM], A[SM], bb[SM];
        tb_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R], S, a, d);
        if (k.method == SLODE_EULER) {
#pragma unroll
          for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s]; bb[s] = h * a[s]; }
        } else if (k.method == SLODE_MIDPOINT) {
          float m[SM], c[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) { m[s] = 1.f - 0.5f * h * d[s]; c[s] = 0.5f * h * a[s]; }
          tb_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 1], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s] * m[s]; bb[s] = h * (a[s] - d[s] * c[s]); }
        } else {   // torchdiffeq's rk4: the 3/8 rule
          const float third = 1.0f / 3.0f, h3 = h * third;
          float p1[SM], q1[SM], p2[SM], q2[SM], c[SM], m[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) { p1[s] = a[s]; q1[s] = -d[s]; c[s] = h3 * p1[s]; m[s] = 1.f + h3 * q1[s]; }
          tb_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 1], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            p2[s] = a[s] - d[s] * c[s]; q2[s] = -d[s] * m[s];
            c[s] = h * (p2[s] - p1[s] * third); m[s] = 1.f + h * (q2[s] - q1[s] * third);
          }
          tb_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 2], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            const float p3 = a[s] - d[s] * c[s], q3 = -d[s] * m[s];
            c[s] = h * (p1[s] - p2[s] + p3); m[s] = 1.f + h * (q1[s] - q2[s] + q3);
            A[s] = q1[s] + 3.f * (q2[s] + q3); bb[s] = p1[s] + 3.f * (p2[s] + p3);   // (partial sums: q4 / p4 follow)
          }
          tb_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 3], S, a, d);
          const float G = h * 0.125f;
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            const float p4 = a[s] - d[s] * c[s], q4 = -d[s] * m[s];
            A[s] = 1.f + G * (A[s] + q4); bb[s] = G * (bb[s] + p4);
          }
        }
#pragma unroll
        for (int s = 0; s < SM; ++s)
          if (s < S) { s_A[n * S + s] = A[s]; s_B[n * S + s] = bb[s]; }
      }
      __syncthreads();
      // ---- B5: forward affine scan, in place: x[n + 1][s] takes the slot of A[n][s] ----
      {
        const int chunk = (NS + 63) / 64, n0 = min(lane * chunk, NS), n1 = min(n0 + chunk, NS);
        for (int s = wave; s < S; s += TB_NT / 64) {
          float* pa = s_A + s;
          const float* pb = s_B + s;
          float Ac = 1.f, bc = 0.f;   // the lane's chunk as one map
          for (int n = n0; n < n1; ++n) { const float An = pa[n * S]; bc = fmaf(An, bc, pb[n * S]); Ac *= An; }
#pragma unroll
          for (int off = 1; off < 64; off <<= 1) {   // inclusive scan of the maps over the lanes (later map o earlier map)
            const float Ap = __shfl_up(Ac, off, 64), bp = __shfl_up(bc, off, 64);
            if (lane >= off) { bc = fmaf(Ac, bp, bc); Ac *= Ap; }
          }
          float Ae = __shfl_up(Ac, 1, 64), be = __shfl_up(bc, 1, 64);
          if (lane == 0) { Ae = 1.f; be = 0.f; }
          float x = fmaf(Ae, s_x0[s], be);
          for (int n = n0; n < n1; ++n) { x = fmaf(pa[n * S], x, pb[n * S]); pa[n * S] = x; }
        }
      }
      __syncthreads();
      // ---- B6: heads + log-likelihood of the thread's time points ----
      float llt = 0.f;
      for (int t = tid; t < T; t += TB_NT) {
        float x[SM];
#pragma unroll
        for (int s = 0; s < SM; ++s) x[s] = s < S ? (t == 0 ? s_x0[s] : s_A[(t - 1) * S + s]) : 0.f;
        float ll = 0.f;
        for (int c = 0; c < C; ++c) {
          const float obv = s_obs[c * T + t], inv = s_inv[c * T + t], lg = s_lg[c * T + t];
          for (int q = 0; q < Q; ++q) {
            float mu = 0.f;
#pragma unroll
            for (int s = 0; s < SM; ++s) if (s < S) mu = fmaf(s_hw[(q * C + c) * S + s], x[s], mu);
            const float r = obv - mu;
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
        const slode_aux ax = k.aux[a];
        const int zd = ax.z_dim, ud = ax.u_dim;
        const float* zz = s_z + ax.z_off;
        const bool unit_on = j32 < U;
        const int jj = min(j32, U - 1);
        float pre = par[k.aux_b1[a] + jj];
        for (int l = 0; l < zd; ++l) pre = fmaf(par[k.aux_w1[a] + jj * zd + l], zz[l], pre);
        const float hv = unit_on ? softplusf(pre) : 0.f;
        float lg[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {   // (columns beyond u_dim add zeros)
          const float w = (q < ud) ? par[k.aux_w2[a] + min(q, ud - 1) * U + jj] : 0.f;
          lg[q] = half_wave_sum(w * hv) + par[k.aux_b2[a] + min(q, ud - 1)];
        }
        float lp = 0.f;
        if (ax.kind == SLODE_AUX_SOFTMAX) {
          float mx = -3.0e38f, se = 0.f;
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) mx = fmaxf(mx, lg[q]);
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) se += expf(lg[q] - mx);
          const float lse = mx + logf(se);
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) lp = fmaf(s_u[ax.u_off + q], lg[q] - lse, lp);
        } else if (ax.kind == SLODE_AUX_SIGMOID) {
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) {
            const float o = lg[q], y = s_u[ax.u_off + q];
            const float sp_pos = (o > 0.f ? o : 0.f) + log1pf(expf(-fabsf(o)));
            lp += y * (o - sp_pos) + (1.f - y) * (-sp_pos);
          }
        } else {   // EXPEXP: Laplace(exp(head 0), softplus(constant_std_*))
          const float bsc = softplusf(par[k.aux_c[a]]), ib = 1.f / bsc;
#pragma unroll
          for (int q = 0; q < 8; ++q) if (q < ud) {
            const float lc = expf(lg[q]), y = s_u[ax.u_off + q];
            lp += -logf(2.f * bsc) - fabsf(y - lc) * ib;
          }
        }
        if (on && j32 == 0) s_item[a] = -k.aux_mult * lp;
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
    tb_reduce_draws(s_loss, s_nll, s_dred, nd, k.B, b, k.bounds, k.loss_kb);
  }
}

// generic: the run-time-S instantiation (rows sized for SLODE_MAX_S)
TbLds tb_lds(const slode_shape& s, int nd, bool generic) {
  auto a4 = [](int v) { return (v + 3) & ~3; };
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3, RW = TB_ROW(generic ? SLODE_MAX_S : s.S), CT = s.C * s.T;
  TbLds o{};
  int n = 0;
  auto take = [&](int c) { const int at = n; n += a4(c); return at; };
  o.a = take((s.T - 1) * s.S); o.b = take((s.T - 1) * s.S); o.obs = take(CT); o.inv = take(CT); o.lg = take(CT); o.row = take(s.H * RW);
  o.w1 = take(s.L * 2 * s.H); o.b1 = take(2 * s.H); o.w2 = take(s.H * s.S + s.S); o.hw = take(Q * s.C * s.S); o.bgd = take(2 * s.S);
  o.z = take(s.L); o.u = take(s.n_u > 0 ? s.n_u : 1); o.h0 = take(s.H); o.x0 = take(s.S); o.item = take(SLODE_MAX_AUX); o.red = take(8);
  o.dred = take(24);   // 12 doubles (the offset is a multiple of 4 floats: 16-byte aligned)
  // the K losses and their likelihood parts come last; a K that cannot fit anyway counts as the whole budget (no overflow of the offsets)
  const int kd = nd < SLODE_TRAJ_BOUNDS_LDS_MAX / 4 ? nd : SLODE_TRAJ_BOUNDS_LDS_MAX / 4;
  o.loss = take(kd); o.nll = take(kd);
  o.total = n;
  return o;
}

}  // namespace

static bool tb_generic(const slode_shape& s, int force_generic) { return force_generic || !(s.S == 5 || s.S == 8); }

size_t slode_traj_bounds_lds_bytes(const slode_shape& s, int num_draws, int force_generic) {
  return (size_t)tb_lds(s, num_draws, tb_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_traj_bounds(const TrajBoundsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  TbK k{};
  k.B = s.B; k.T = s.T; k.C = s.C; k.L = s.L; k.S = s.S; k.H = s.H; k.nu = s.n_u; k.n_groups = s.n_groups; k.n_aux = s.n_aux; k.U = s.U;
  k.method = s.method; k.R = s.method == SLODE_EULER ? 1 : (s.method == SLODE_MIDPOINT ? 2 : 3);
  k.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; k.Q = k.gauss ? 1 : 3;
  k.nd = a.num_draws; k.t_major = a.t_major;
  k.aux_mult = s.aux_mult; k.tau[0] = 0.5f; k.tau[1] = 0.5f + s.quantile_diff; k.tau[2] = 0.5f - s.quantile_diff;
  for (int g = 0; g < SLODE_MAX_GROUPS; ++g) {
    k.grp[g] = s.groups[g]; k.ploc_w[g] = lay.ploc_w[g]; k.ploc_b[g] = lay.ploc_b[g]; k.pls_w[g] = lay.pls_w[g]; k.pls_b[g] = lay.pls_b[g];
  }
  for (int q = 0; q < SLODE_MAX_AUX; ++q) {
    k.aux[q] = s.aux[q]; k.aux_w1[q] = lay.aux_w1[q]; k.aux_b1[q] = lay.aux_b1[q]; k.aux_w2[q] = lay.aux_w2[q]; k.aux_b2[q] = lay.aux_b2[q];
    k.aux_c[q] = lay.aux_c[q];
  }
  k.init_w1 = lay.init_w1; k.init_b1 = lay.init_b1; k.init_w2 = lay.init_w2; k.init_b2 = lay.init_b2;
  k.dyn_wh = lay.dyn_wh; k.dyn_bh = lay.dyn_bh; k.dyn_wg = lay.dyn_wg; k.dyn_bg = lay.dyn_bg; k.dyn_wd = lay.dyn_wd; k.dyn_bd = lay.dyn_bd;
  for (int q = 0; q < SLODE_MAX_HEADS; ++q) k.head[q] = lay.head_w[q];
  k.params = a.params; k.times = a.times; k.stage_t = a.stage_t; k.obs = a.obs; k.sb = a.sb;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u; k.sigtab = a.sigtab; k.bounds = a.bounds; k.loss_kb = a.loss_kb;
  k.rng = a.rng; k.lab = a.lab; k.o = tb_lds(s, a.num_draws, tb_generic(s, a.force_generic));
  const size_t lds = slode_traj_bounds_lds_bytes(s, a.num_draws, a.force_generic);
  if (lds > SLODE_TRAJ_BOUNDS_LDS_MAX || a.num_draws < 1 || a.grid < 1 || s.n_aux > SLODE_MAX_AUX) return hipErrorInvalidValue;
#define SLODE_TB_GO(SC, LAB)                                                                                                             \
  do {                                                                                                                                   \
    auto fn_ = traj_bounds_kernel<SC, LAB>;                                                                                              \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)fn_, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);               \
    SLODE_LAUNCH("traj_bounds", fn_, dim3(a.grid), dim3(TB_NT), lds, stream, k);                                                          \
  } while (0)
  const bool lab = s.aux_in_main && s.n_aux > 0;
  if (tb_generic(s, a.force_generic)) { if (lab) SLODE_TB_GO(0, true); else SLODE_TB_GO(0, false); }
  else if (s.S == 5) { if (lab) SLODE_TB_GO(5, true); else SLODE_TB_GO(5, false); }
  else { if (lab) SLODE_TB_GO(8, true); else SLODE_TB_GO(8, false); }
#undef SLODE_TB_GO
  return hipGetLastError();
}
