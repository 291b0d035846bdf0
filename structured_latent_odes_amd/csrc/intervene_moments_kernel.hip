// Counterfactual curves (slode_intervene_moments): per trajectory, over num_samples PAIRED latent draws, the mean and the population standard
// deviation of every decoder head curve under swapped labels (v_cf) and of its difference to the subject's own curve (v_cf - v_f) -- without
// writing anything sized num_samples x B x C x T.  Both arms of a draw share ONE noise row:
//   factual         z_f  = loc_q(x_b) + scale_q(x_b) * eps                       (the posterior draw of recon_moments_kernel, is_post)
//   counterfactual  z_cf = z_f outside every intervened prior group; inside group g: ploc_g(u'_b) + exp(pls_g(u'_b)) * eps
// The forward phases are those of recon_moments_kernel.hip (M0-M7), restated here; M3-M6 run once per arm.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in order:
//   M0  once per workgroup: [w_t | u_j | W_g | W_d] per hidden unit, the z-columns of the hidden layer and the init net (transposed), the
//       init net's output layer, the head weights and the biases into the LDS -- both arms of every draw of every trajectory reuse them
//   M1  once per trajectory: the counterfactual labels of the intervened groups; per latent dim the posterior loc / scale (from the encoder
//       launch) and the counterfactual loc / scale (the group's conditional prior nets on u' inside an intervened group, else the posterior's)
//   per draw: one noise value per latent dim (row k * B + b of ONE drawing call, or of the explicit [ns, B, L] tensor), kept by its thread
//   per arm (factual, then counterfactual):
//   M2  z = loc + scale * eps_k with the arm's loc / scale
//   M3  time-invariant part of the hidden layer (into the unit's weight row) and the init net; x0
//   M4  step coefficients x' = A x + b of every grid step (tests/kernel_math.py step_coeffs), thread <-> step, weights from the LDS
//   M5  forward affine scan (one solve on all four waves): one state component per wave pass
//   M6  thread <-> time point: the Q * C head values v.  Factual arm: kept in the LDS ([Q*C][T], the thread's own slots).  Counterfactual arm:
//       two sets of running moments of (q, c, t), each shifted by its first draw's value: of v_cf and of e = v_cf - v_f
//       (s1 += v - v0, s2 += (v - v0)^2 -- no sum of squares of the values themselves)
//   M7  once per trajectory: mean = v0 + s1 / ns, sd = sqrt(max(0, s2 - s1^2 / ns) / ns) of both sets, written with T contiguous
// The moments (and the kept factual values) of (q, c, t) belong to ONE thread for the whole trajectory, which takes the draws in the fixed
// order k = 0 .. ns - 1: the result is a function of (parameters, inputs, labels, noise) alone -- independent of the grid, bitwise
// reproducible, no atomics.  With no group intervened both arms run the same operations on the same z: the effect is exactly 0.
#include "slode_common.h"

namespace {

constexpr int IV_NT = 256;
#define IV_ROW(SM) ((2 + 2 * (SM) + 3) & ~3)   // floats of one hidden unit's LDS row: w_t | u_j | W_g[0..SM) | W_d[0..SM)

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region
struct IvLds { int a, b, acc, vf, row, w1, b1, w2, hw, bgd, z, loc, sc, cloc, csc, u, h0, x0, total; };

struct IvK {
  int B, T, C, L, S, H, nu, n_groups, R, method, Q, ns, mask;
  slode_group grp[SLODE_MAX_GROUPS];
  int ploc_w[SLODE_MAX_GROUPS], ploc_b[SLODE_MAX_GROUPS], pls_w[SLODE_MAX_GROUPS], pls_b[SLODE_MAX_GROUPS];
  int init_w1, init_b1, init_w2, init_b2, dyn_wh, dyn_bh, dyn_wg, dyn_bg, dyn_wd, dyn_bd, head[SLODE_MAX_HEADS];
  const float *params, *times, *stage_t, *loc, *scale, *eps;
  float *cf_mean, *cf_sd, *eff_mean, *eff_sd;
  IvLds o;
  RngK rng;
  LabelSrc cf;   // the counterfactual label tensors, one by one (n >= 1 whenever mask != 0)
};

// a(t, z), d(t, z) of one stage time from the LDS rows [w_t | u_j | W_g[.][j] | W_d[.][j]] (every lane reads the same address: broadcast)
// (rows are RW = 2 + 2 SM floats rounded up to a multiple of four, 16-byte aligned: read as 16-byte LDS loads)
template <int SM>
__device__ __forceinline__ void iv_ad(const float* __restrict__ s_row, const float* __restrict__ s_bgd, int H, float t, int S,
                                      float (&a)[SM], float (&d)[SM]) {
  typedef float f4_t __attribute__((ext_vector_type(4)));
  constexpr int RW = IV_ROW(SM);
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

// one running moment set [v0 | s1 | s2] (T floats apart) of the thread's (q, c, t), draw kk
__device__ __forceinline__ void iv_moment(float* m, int T, int kk, float v) {
  if (kk == 0) { m[0] = v; m[T] = 0.f; m[2 * T] = 0.f; }
  else { const float dv = v - m[0]; m[T] += dv; m[2 * T] = fmaf(dv, dv, m[2 * T]); }
}

// column `col` of u' from the counterfactual label tensors (slode_label_at without the one-dense-matrix form, which this call does not take)
__device__ __forceinline__ float iv_label_at(const LabelSrc& ls, long long b, int col) {
  int i = 0;
#pragma unroll
  for (int q = 1; q < SLODE_MAX_LABELS; ++q) i = (q < ls.n && col >= ls.off[q]) ? q : i;
  const int w = ls.off[i + 1] - ls.off[i];
  return ls.p[i][b * w + (col - ls.off[i])];
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(IV_NT) intervene_moments_kernel(const IvK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_iv[];
  const float* __restrict__ par = k.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = k.T, L = k.L, S = SC ? SC : k.S, H = k.H, C = k.C, Q = k.Q, NS = T - 1, QC = Q * C, ns = k.ns;
  constexpr int RW = IV_ROW(SM);
  float* s_A = s_iv + k.o.a;       // A[T-1][S], overwritten by x[n+1][.] in the scan
  float* s_B = s_iv + k.o.b;       // b[T-1][S]
  float* s_acc = s_iv + k.o.acc;   // [Q*C][6: v0, s1, s2 of v_cf | v0, s1, s2 of v_cf - v_f][T]
  float* s_vf = s_iv + k.o.vf;     // [Q*C][T]: the factual head values of the current draw
  float* s_row = s_iv + k.o.row;   // [H][RW]: w_t | u_j (per arm of a draw) | W_g[0..S)[j] | W_d[0..S)[j]
  float* s_w1 = s_iv + k.o.w1;     // [L][2H]: z-columns of the hidden layer (r < H) and the init net's first layer (r >= H), transposed
  float* s_b1 = s_iv + k.o.b1;     // [2H]
  float* s_w2 = s_iv + k.o.w2;     // [H][S] init net's output layer, transposed | [S] its bias
  float* s_hw = s_iv + k.o.hw;     // [Q*C][S] head weights
  float* s_bgd = s_iv + k.o.bgd;   // [2S] growth | degradation bias
  float* s_z = s_iv + k.o.z;
  float* s_loc = s_iv + k.o.loc;   // posterior loc / scale
  float* s_sc = s_iv + k.o.sc;
  float* s_cloc = s_iv + k.o.cloc; // counterfactual loc / scale
  float* s_csc = s_iv + k.o.csc;
  float* s_u = s_iv + k.o.u;       // u' (only the columns of intervened groups are filled and read)
  float* s_h0 = s_iv + k.o.h0;
  float* s_x0 = s_iv + k.o.x0;
  const bool need_f = k.eff_mean || k.eff_sd;   // (workgroup-uniform: the factual arm serves the effect alone)

  // ---- M0: the weights every solve reuses ----
  for (int i = tid; i < H * RW; i += IV_NT) {
    const int j = i / RW, c = i - j * RW;
    float v = 0.f;
    if (c == 0) v = par[k.dyn_wh + j * (1 + L)];
    else if (c >= 2 && c < 2 + S) v = par[k.dyn_wg + (c - 2) * H + j];
    else if (c >= 2 + SM && c < 2 + SM + S) v = par[k.dyn_wd + (c - 2 - SM) * H + j];
    s_row[i] = v;
  }
  for (int i = tid; i < L * 2 * H; i += IV_NT) {
    const int l = i / (2 * H), r = i - l * 2 * H;
    s_w1[i] = r < H ? par[k.dyn_wh + r * (1 + L) + 1 + l] : par[k.init_w1 + (r - H) * L + l];
  }
  for (int i = tid; i < 2 * H; i += IV_NT) s_b1[i] = i < H ? par[k.dyn_bh + i] : par[k.init_b1 + i - H];
  for (int i = tid; i < H * S + S; i += IV_NT) {
    const int j = i / S, s = i - j * S;
    s_w2[i] = i < H * S ? par[k.init_w2 + s * H + j] : par[k.init_b2 + i - H * S];
  }
  for (int i = tid; i < QC * S; i += IV_NT) {
    const int qc = i / S, q = qc / C;
    s_hw[i] = par[k.head[q] + (qc - q * C) * S + (i - qc * S)];
  }
  for (int i = tid; i < 2 * S; i += IV_NT) s_bgd[i] = i < S ? par[k.dyn_bg + i] : par[k.dyn_bd + i - S];

  for (int b = blockIdx.x; b < k.B; b += gridDim.x) {
    // ---- M1 ----
    __syncthreads();   // (M0's writes; the previous trajectory's readers of s_u / s_loc / s_sc / s_cloc / s_csc)
    if (tid < k.nu) {
      int hit = 0;
      for (int g = 0; g < k.n_groups; ++g)
        if (((k.mask >> g) & 1) && tid >= k.grp[g].u_off && tid < k.grp[g].u_off + k.grp[g].u_dim) hit = 1;
      if (hit) s_u[tid] = iv_label_at(k.cf, b, tid);
    }
    __syncthreads();
    if (tid < L) {
      const int l = tid;
      const float loc = k.loc[(long long)b * L + l], sc = k.scale[(long long)b * L + l];
      float cloc = loc, csc = sc;
      for (int g = 0; g < k.n_groups; ++g) {
        const slode_group gr = k.grp[g];
        if (((k.mask >> g) & 1) && l >= gr.z_off && l < gr.z_off + gr.z_dim) {
          const int ll = l - gr.z_off;
          float pl = par[k.ploc_b[g] + ll], pls = par[k.pls_b[g] + ll];
          for (int q = 0; q < gr.u_dim; ++q) {
            const float uv = s_u[gr.u_off + q];
            pl = fmaf(par[k.ploc_w[g] + ll * gr.u_dim + q], uv, pl);
            pls = fmaf(par[k.pls_w[g] + ll * gr.u_dim + q], uv, pls);
          }
          cloc = pl; csc = expf(pls);
        }
      }
      s_loc[l] = loc; s_sc[l] = sc; s_cloc[l] = cloc; s_csc[l] = csc;   // (read back by this thread alone)
    }
    for (int kk = 0; kk < ns; ++kk) {
      // draw kk = row kk * B + b of the call's noise: ONE value per latent dim, shared by both arms
      const float e = tid < L ? slode_eps_at(k.rng, k.eps, (long long)kk * k.B + b, L, tid) : 0.f;
      for (int arm = need_f ? 0 : 1; arm < 2; ++arm) {
        // ---- M2 ----
        if (tid < L) s_z[tid] = arm ? fmaf(s_csc[tid], e, s_cloc[tid]) : fmaf(s_sc[tid], e, s_loc[tid]);
        __syncthreads();   // (also: the previous solve's readers of s_A / s_x0 / s_row[.][1] are done)
        // ---- M3: u = W_z z + b_h into the units' rows; the init net's hidden layer ----
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
        // ---- M4: step coefficients ----
        for (int n = tid; n < NS; n += IV_NT) {
          const float h = k.times[n + 1] - k.times[n];
          float a[SM], d[SM], A[SM], bb[SM];
          iv_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R], S, a, d);
          if (k.method == SLODE_EULER) {
#pragma unroll
            for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s]; bb[s] = h * a[s]; }
          } else if (k.method == SLODE_MIDPOINT) {
            float m[SM], c[SM];
#pragma unroll
            for (int s = 0; s < SM; ++s) { m[s] = 1.f - 0.5f * h * d[s]; c[s] = 0.5f * h * a[s]; }
            iv_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 1], S, a, d);
#pragma unroll
            for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s] * m[s]; bb[s] = h * (a[s] - d[s] * c[s]); }
          } else {   // torchdiffeq's rk4: the 3/8 rule
            const float third = 1.0f / 3.0f, h3 = h * third;
            float p1[SM], q1[SM], p2[SM], q2[SM], c[SM], m[SM];
#pragma unroll
            for (int s = 0; s < SM; ++s) { p1[s] = a[s]; q1[s] = -d[s]; c[s] = h3 * p1[s]; m[s] = 1.f + h3 * q1[s]; }
            iv_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 1], S, a, d);
#pragma unroll
            for (int s = 0; s < SM; ++s) {
              p2[s] = a[s] - d[s] * c[s]; q2[s] = -d[s] * m[s];
              c[s] = h * (p2[s] - p1[s] * third); m[s] = 1.f + h * (q2[s] - q1[s] * third);
            }
            iv_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 2], S, a, d);
#pragma unroll
            for (int s = 0; s < SM; ++s) {
              const float p3 = a[s] - d[s] * c[s], q3 = -d[s] * m[s];
              c[s] = h * (p1[s] - p2[s] + p3); m[s] = 1.f + h * (q1[s] - q2[s] + q3);
              A[s] = q1[s] + 3.f * (q2[s] + q3); bb[s] = p1[s] + 3.f * (p2[s] + p3);   // (partial sums: q4 / p4 follow)
            }
            iv_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 3], S, a, d);
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
        // ---- M5: forward affine scan, in place: x[n + 1][s] takes the slot of A[n][s] ----
        {
          const int chunk = (NS + 63) / 64, n0 = min(lane * chunk, NS), n1 = min(n0 + chunk, NS);
          for (int s = wave; s < S; s += IV_NT / 64) {
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
        // ---- M6: head values of the thread's time points; factual: kept; counterfactual: both running moment sets ----
        for (int t = tid; t < T; t += IV_NT) {
          float x[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) x[s] = s < S ? (t == 0 ? s_x0[s] : s_A[(t - 1) * S + s]) : 0.f;
          for (int qc = 0; qc < QC; ++qc) {
            float v = 0.f;
#pragma unroll
            for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(s_hw[qc * S + s], x[s], v);
            if (arm == 0) {
              s_vf[qc * T + t] = v;
            } else {
              float* m = s_acc + (qc * 6) * T + t;
              iv_moment(m, T, kk, v);
              if (need_f) iv_moment(m + 3 * T, T, kk, v - s_vf[qc * T + t]);
            }
          }
        }
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    {
      const float inv = 1.0f / (float)ns;
      for (int t = tid; t < T; t += IV_NT)
        for (int qc = 0; qc < QC; ++qc) {
          const int q = qc / C, c = qc - q * C;
          const float* m = s_acc + (qc * 6) * T + t;
          const long long o = (((long long)q * k.B + b) * C + c) * T + t;
          {
            const float s1 = m[T], s2 = m[2 * T];
            if (k.cf_mean) k.cf_mean[o] = fmaf(s1, inv, m[0]);
            if (k.cf_sd) k.cf_sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
          }
          if (need_f) {
            const float s1 = m[4 * T], s2 = m[5 * T];
            if (k.eff_mean) k.eff_mean[o] = fmaf(s1, inv, m[3 * T]);
            if (k.eff_sd) k.eff_sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
          }
        }
    }
  }
}

// generic: the run-time-S instantiation (rows sized for SLODE_MAX_S)
IvLds iv_lds(const slode_shape& s, bool generic) {
  auto a4 = [](int v) { return (v + 3) & ~3; };
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3, RW = IV_ROW(generic ? SLODE_MAX_S : s.S);
  IvLds o{};
  int n = 0;
  auto take = [&](int c) { const int at = n; n += a4(c); return at; };
  o.a = take((s.T - 1) * s.S); o.b = take((s.T - 1) * s.S); o.acc = take(Q * s.C * 6 * s.T); o.vf = take(Q * s.C * s.T); o.row = take(s.H * RW);
  o.w1 = take(s.L * 2 * s.H); o.b1 = take(2 * s.H); o.w2 = take(s.H * s.S + s.S); o.hw = take(Q * s.C * s.S); o.bgd = take(2 * s.S);
  o.z = take(s.L); o.loc = take(s.L); o.sc = take(s.L); o.cloc = take(s.L); o.csc = take(s.L); o.u = take(s.n_u > 0 ? s.n_u : 1);
  o.h0 = take(s.H); o.x0 = take(s.S);
  o.total = n;
  return o;
}

}  // namespace

static bool iv_generic(const slode_shape& s, int force_generic) { return force_generic || !(s.S == 5 || s.S == 8); }

size_t slode_intervene_moments_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)iv_lds(s, iv_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_intervene_moments(const InterveneMomentsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  IvK k{};
  k.B = s.B; k.T = s.T; k.C = s.C; k.L = s.L; k.S = s.S; k.H = s.H; k.nu = s.n_u; k.n_groups = s.n_groups;
  k.method = s.method; k.R = s.method == SLODE_EULER ? 1 : (s.method == SLODE_MIDPOINT ? 2 : 3);
  k.Q = s.likelihood == SLODE_GAUSS ? 1 : 3; k.ns = a.num_samples; k.mask = (int)a.group_mask;
  for (int g = 0; g < SLODE_MAX_GROUPS; ++g) {
    k.grp[g] = s.groups[g]; k.ploc_w[g] = lay.ploc_w[g]; k.ploc_b[g] = lay.ploc_b[g]; k.pls_w[g] = lay.pls_w[g]; k.pls_b[g] = lay.pls_b[g];
  }
  k.init_w1 = lay.init_w1; k.init_b1 = lay.init_b1; k.init_w2 = lay.init_w2; k.init_b2 = lay.init_b2;
  k.dyn_wh = lay.dyn_wh; k.dyn_bh = lay.dyn_bh; k.dyn_wg = lay.dyn_wg; k.dyn_bg = lay.dyn_bg; k.dyn_wd = lay.dyn_wd; k.dyn_bd = lay.dyn_bd;
  for (int q = 0; q < SLODE_MAX_HEADS; ++q) k.head[q] = lay.head_w[q];
  k.params = a.params; k.times = a.times; k.stage_t = a.stage_t; k.loc = a.loc; k.scale = a.scale; k.eps = a.eps;
  k.cf_mean = a.cf_mean; k.cf_sd = a.cf_sd; k.eff_mean = a.eff_mean; k.eff_sd = a.eff_sd;
  k.rng = a.rng; k.cf = a.cf; k.o = iv_lds(s, iv_generic(s, a.force_generic));
  const size_t lds = slode_intervene_moments_lds_bytes(s, a.force_generic);
  if (lds > SLODE_INTERVENE_MOMENTS_LDS_MAX || a.num_samples < 1 || a.grid < 1 || (a.group_mask != 0 && a.cf.n < 1)) return hipErrorInvalidValue;
#define SLODE_IV_GO(SC)                                                                                                                    \
  do {                                                                                                                                     \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)intervene_moments_kernel<SC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    SLODE_LAUNCH("intervene_moments", intervene_moments_kernel<SC>, dim3(a.grid), dim3(IV_NT), lds, stream, k);                             \
  } while (0)
  if (iv_generic(s, a.force_generic)) SLODE_IV_GO(0);
  else if (s.S == 5) SLODE_IV_GO(5);
  else SLODE_IV_GO(8);
#undef SLODE_IV_GO
  return hipGetLastError();
}
