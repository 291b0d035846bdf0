// Sample moments of the reconstruction (slode_recon_moments): per trajectory, the mean and the population standard deviation over
// num_samples latent draws of every decoder head curve -- what the reference's evaluation takes from `multiple_samples` (np.mean / np.std
// over the sample axis) -- without writing anything sized num_samples x B x C x T.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in
// that order:
//   M0  once per workgroup: [w_t | u_j | W_g | W_d] per hidden unit, the z-columns of the hidden layer and the init net (transposed), the
//       init net's output layer, the head weights and the biases into the LDS -- every draw of every trajectory reuses them
//   M1  once per trajectory: labels; loc / scale of the posterior (from the encoder launch) or of the conditional prior nets, N(0, 1) on
//       the dims outside every prior group (as phase E0 of eval_stats_kernel forms z3)
//   per draw:
//   M2  z = loc + scale * eps_k (row k * B + b of ONE drawing call, or of the explicit [ns, B, L] tensor)
//   M3  time-invariant part of the hidden layer (into the unit's weight row) and the init net; x0
//   M4  step coefficients x' = A x + b of every grid step (tests/kernel_math.py step_coeffs), thread <-> step, weights from the LDS
//   M5  forward affine scan (phases E1-E3 of eval_kernel.hip, one solve on all four waves): one state component per wave pass
//   M6  thread <-> time point: the Q * C head values v and the running moments of (q, c, t), shifted by the first draw's value v0:
//       s1 += v - v0, s2 += (v - v0)^2 -- no sum of v^2, whose fp32 rounding would exceed the variance of a prior-pass curve
//   M7  once per trajectory: mean = v0 + s1 / ns, sd = sqrt(max(0, s2 - s1^2 / ns) / ns), written with T contiguous
// The moments of (q, c, t) belong to ONE thread for the whole trajectory and take the draws in the fixed order k = 0 .. ns - 1: the
// result is a function of (parameters, inputs, noise) alone -- independent of the grid, bitwise reproducible, no atomics.
#include "slode_common.h"

namespace {

constexpr int RM_NT = 256;
#define RM_ROW(SM) ((2 + 2 * (SM) + 3) & ~3)   // floats of one hidden unit's LDS row: w_t | u_j | W_g[0..SM) | W_d[0..SM)

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region
struct RmLds { int a, b, acc, row, w1, b1, w2, hw, bgd, z, loc, sc, u, h0, x0, total; };

struct RmK {
  int B, T, C, L, S, H, nu, n_groups, R, method, is_post, Q, ns;
  slode_group grp[SLODE_MAX_GROUPS];
  int ploc_w[SLODE_MAX_GROUPS], ploc_b[SLODE_MAX_GROUPS], pls_w[SLODE_MAX_GROUPS], pls_b[SLODE_MAX_GROUPS];
  int init_w1, init_b1, init_w2, init_b2, dyn_wh, dyn_bh, dyn_wg, dyn_bg, dyn_wd, dyn_bd, head[SLODE_MAX_HEADS];
  const float *params, *times, *stage_t, *loc, *scale, *eps, *u;
  float *mean, *sd;
  RmLds o;
  RngK rng;
  LabelSrc lab;
};

// a(t, z), d(t, z) of one stage time from the LDS rows [w_t | u_j | W_g[.][j] | W_d[.][j]] (every lane reads the same address: broadcast)
// (rows are RW = 2 + 2 SM floats rounded up to a multiple of four, 16-byte aligned: read as 16-byte LDS loads)
template <int SM>
__device__ __forceinline__ void rm_ad(const float* __restrict__ s_row, const float* __restrict__ s_bgd, int H, float t, int S,
                                      float (&a)[SM], float (&d)[SM]) {
  typedef float f4_t __attribute__((ext_vector_type(4)));
  constexpr int RW = RM_ROW(SM);
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

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(RM_NT) recon_moments_kernel(const RmK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_rm[];
  const float* __restrict__ par = k.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int T = k.T, L = k.L, S = SC ? SC : k.S, H = k.H, C = k.C, Q = k.Q, NS = T - 1, QC = Q * C, ns = k.ns;
  constexpr int RW = RM_ROW(SM);
  float* s_A = s_rm + k.o.a;       // A[T-1][S], overwritten by x[n+1][.] in the scan
  float* s_B = s_rm + k.o.b;       // b[T-1][S]
  float* s_acc = s_rm + k.o.acc;   // [Q*C][3: v0, s1, s2][T]
  float* s_row = s_rm + k.o.row;   // [H][RW]: w_t | u_j (per draw) | W_g[0..S)[j] | W_d[0..S)[j]
  float* s_w1 = s_rm + k.o.w1;     // [L][2H]: z-columns of the hidden layer (r < H) and the init net's first layer (r >= H), transposed
  float* s_b1 = s_rm + k.o.b1;     // [2H]
  float* s_w2 = s_rm + k.o.w2;     // [H][S] init net's output layer, transposed | [S] its bias
  float* s_hw = s_rm + k.o.hw;     // [Q*C][S] head weights
  float* s_bgd = s_rm + k.o.bgd;   // [2S] growth | degradation bias
  float* s_z = s_rm + k.o.z;
  float* s_loc = s_rm + k.o.loc;
  float* s_sc = s_rm + k.o.sc;
  float* s_u = s_rm + k.o.u;
  float* s_h0 = s_rm + k.o.h0;
  float* s_x0 = s_rm + k.o.x0;

  // ---- M0: the weights every draw reuses ----
  for (int i = tid; i < H * RW; i += RM_NT) {
    const int j = i / RW, c = i - j * RW;
    float v = 0.f;
    if (c == 0) v = par[k.dyn_wh + j * (1 + L)];
    else if (c >= 2 && c < 2 + S) v = par[k.dyn_wg + (c - 2) * H + j];
    else if (c >= 2 + SM && c < 2 + SM + S) v = par[k.dyn_wd + (c - 2 - SM) * H + j];
    s_row[i] = v;
  }
  for (int i = tid; i < L * 2 * H; i += RM_NT) {
    const int l = i / (2 * H), r = i - l * 2 * H;
    s_w1[i] = r < H ? par[k.dyn_wh + r * (1 + L) + 1 + l] : par[k.init_w1 + (r - H) * L + l];
  }
  for (int i = tid; i < 2 * H; i += RM_NT) s_b1[i] = i < H ? par[k.dyn_bh + i] : par[k.init_b1 + i - H];
  for (int i = tid; i < H * S + S; i += RM_NT) {
    const int j = i / S, s = i - j * S;
    s_w2[i] = i < H * S ? par[k.init_w2 + s * H + j] : par[k.init_b2 + i - H * S];
  }
  for (int i = tid; i < QC * S; i += RM_NT) {
    const int qc = i / S, q = qc / C;
    s_hw[i] = par[k.head[q] + (qc - q * C) * S + (i - qc * S)];
  }
  for (int i = tid; i < 2 * S; i += RM_NT) s_bgd[i] = i < S ? par[k.dyn_bg + i] : par[k.dyn_bd + i - S];

  for (int b = blockIdx.x; b < k.B; b += gridDim.x) {
    // ---- M1 ----
    __syncthreads();   // (M0's writes; the previous trajectory's readers of s_u / s_loc / s_sc)
    if (!k.is_post && k.n_groups > 0 && tid < k.nu) s_u[tid] = slode_label_at(k.lab, k.u, k.nu, b, tid);   // (only the conditional prior nets read labels)
    __syncthreads();
    if (tid < L) {
      const int l = tid;
      float loc, sc;
      if (k.is_post) {
        loc = k.loc[(long long)b * L + l]; sc = k.scale[(long long)b * L + l];
      } else {
        float pl = 0.f, pls = 0.f;
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
        loc = pl; sc = expf(pls);
      }
      s_loc[l] = loc; s_sc[l] = sc;
    }
    for (int kk = 0; kk < ns; ++kk) {
      // ---- M2: draw kk = row kk * B + b of the call's noise ----
      if (tid < L) s_z[tid] = fmaf(s_sc[tid], slode_eps_at(k.rng, k.eps, (long long)kk * k.B + b, L, tid), s_loc[tid]);
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
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
      for (int n = tid; n < NS; n += RM_NT) {
        const float h = k.times[n + 1] - k.times[n];
        float a[SM], d[SM], A[SM], bb[SM];
        rm_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R], S, a, d);
        if (k.method == SLODE_EULER) {
#pragma unroll
          for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s]; bb[s] = h * a[s]; }
        } else if (k.method == SLODE_MIDPOINT) {
          float m[SM], c[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) { m[s] = 1.f - 0.5f * h * d[s]; c[s] = 0.5f * h * a[s]; }
          rm_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 1], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s] * m[s]; bb[s] = h * (a[s] - d[s] * c[s]); }
        } else {   // torchdiffeq's rk4: the 3/8 rule
          const float third = 1.0f / 3.0f, h3 = h * third;
          float p1[SM], q1[SM], p2[SM], q2[SM], c[SM], m[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) { p1[s] = a[s]; q1[s] = -d[s]; c[s] = h3 * p1[s]; m[s] = 1.f + h3 * q1[s]; }
          rm_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 1], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            p2[s] = a[s] - d[s] * c[s]; q2[s] = -d[s] * m[s];
            c[s] = h * (p2[s] - p1[s] * third); m[s] = 1.f + h * (q2[s] - q1[s] * third);
          }
          rm_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 2], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            const float p3 = a[s] - d[s] * c[s], q3 = -d[s] * m[s];
            c[s] = h * (p1[s] - p2[s] + p3); m[s] = 1.f + h * (q1[s] - q2[s] + q3);
            A[s] = q1[s] + 3.f * (q2[s] + q3); bb[s] = p1[s] + 3.f * (p2[s] + p3);   // (partial sums: q4 / p4 follow)
          }
          rm_ad<SM>(s_row, s_bgd, H, k.stage_t[n * k.R + 3], S, a, d);
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
        for (int s = wave; s < S; s += RM_NT / 64) {
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
      // ---- M6: head values of the thread's time points, running moments ----
      for (int t = tid; t < T; t += RM_NT) {
        float x[SM];
#pragma unroll
        for (int s = 0; s < SM; ++s) x[s] = s < S ? (t == 0 ? s_x0[s] : s_A[(t - 1) * S + s]) : 0.f;
        for (int qc = 0; qc < QC; ++qc) {
          float v = 0.f;
#pragma unroll
          for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(s_hw[qc * S + s], x[s], v);
          float* m = s_acc + (qc * 3) * T + t;
          if (kk == 0) { m[0] = v; m[T] = 0.f; m[2 * T] = 0.f; }
          else { const float dv = v - m[0]; m[T] += dv; m[2 * T] = fmaf(dv, dv, m[2 * T]); }
        }
      }
    }
    // ---- M7: the thread's own (q, c, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    {
      const float inv = 1.0f / (float)ns;
      for (int t = tid; t < T; t += RM_NT)
        for (int qc = 0; qc < QC; ++qc) {
          const int q = qc / C, c = qc - q * C;
          const float* m = s_acc + (qc * 3) * T + t;
          const float s1 = m[T], s2 = m[2 * T];
          const long long o = (((long long)q * k.B + b) * C + c) * T + t;
          k.mean[o] = fmaf(s1, inv, m[0]);
          if (k.sd) k.sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
        }
    }
  }
}

// generic: the run-time-S instantiation (rows sized for SLODE_MAX_S)
RmLds rm_lds(const slode_shape& s, bool generic) {
  auto a4 = [](int v) { return (v + 3) & ~3; };
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3, RW = RM_ROW(generic ? SLODE_MAX_S : s.S);
  RmLds o{};
  int n = 0;
  auto take = [&](int c) { const int at = n; n += a4(c); return at; };
  o.a = take((s.T - 1) * s.S); o.b = take((s.T - 1) * s.S); o.acc = take(Q * s.C * 3 * s.T); o.row = take(s.H * RW);
  o.w1 = take(s.L * 2 * s.H); o.b1 = take(2 * s.H); o.w2 = take(s.H * s.S + s.S); o.hw = take(Q * s.C * s.S); o.bgd = take(2 * s.S);
  o.z = take(s.L); o.loc = take(s.L); o.sc = take(s.L); o.u = take(s.n_u > 0 ? s.n_u : 1); o.h0 = take(s.H); o.x0 = take(s.S);
  o.total = n;
  return o;
}

}  // namespace

static bool rm_generic(const slode_shape& s, int force_generic) { return force_generic || !(s.S == 5 || s.S == 8); }

size_t slode_recon_moments_lds_bytes(const slode_shape& s, int force_generic) {
  return (size_t)rm_lds(s, rm_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_recon_moments(const ReconMomentsLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  RmK k{};
  k.B = s.B; k.T = s.T; k.C = s.C; k.L = s.L; k.S = s.S; k.H = s.H; k.nu = s.n_u; k.n_groups = s.n_groups;
  k.method = s.method; k.R = s.method == SLODE_EULER ? 1 : (s.method == SLODE_MIDPOINT ? 2 : 3);
  k.Q = s.likelihood == SLODE_GAUSS ? 1 : 3; k.is_post = a.is_post; k.ns = a.num_samples;
  for (int g = 0; g < SLODE_MAX_GROUPS; ++g) {
    k.grp[g] = s.groups[g]; k.ploc_w[g] = lay.ploc_w[g]; k.ploc_b[g] = lay.ploc_b[g]; k.pls_w[g] = lay.pls_w[g]; k.pls_b[g] = lay.pls_b[g];
  }
  k.init_w1 = lay.init_w1; k.init_b1 = lay.init_b1; k.init_w2 = lay.init_w2; k.init_b2 = lay.init_b2;
  k.dyn_wh = lay.dyn_wh; k.dyn_bh = lay.dyn_bh; k.dyn_wg = lay.dyn_wg; k.dyn_bg = lay.dyn_bg; k.dyn_wd = lay.dyn_wd; k.dyn_bd = lay.dyn_bd;
  for (int q = 0; q < SLODE_MAX_HEADS; ++q) k.head[q] = lay.head_w[q];
  k.params = a.params; k.times = a.times; k.stage_t = a.stage_t; k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u;
  k.mean = a.mean; k.sd = a.sd; k.rng = a.rng; k.lab = a.lab; k.o = rm_lds(s, rm_generic(s, a.force_generic));
  const size_t lds = slode_recon_moments_lds_bytes(s, a.force_generic);
  if (lds > SLODE_RECON_MOMENTS_LDS_MAX || a.num_samples < 1 || a.grid < 1) return hipErrorInvalidValue;
#define SLODE_RM_GO(SC)                                                                                                                    \
  do {                                                                                                                                     \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)recon_moments_kernel<SC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    SLODE_LAUNCH("recon_moments", recon_moments_kernel<SC>, dim3(a.grid), dim3(RM_NT), lds, stream, k);                                     \
  } while (0)
  if (rm_generic(s, a.force_generic)) SLODE_RM_GO(0);
  else if (s.S == 5) SLODE_RM_GO(5);
  else SLODE_RM_GO(8);
#undef SLODE_RM_GO
  return hipGetLastError();
}
