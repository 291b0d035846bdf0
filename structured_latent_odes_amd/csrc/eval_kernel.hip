// Fused statistics pass (slode_eval_stats): what one batch of the reference's per-epoch statistics needs -- the -ELBO of the main loss, the
// auxiliary loss, the reconstruction L1 of one more latent draw and the label-prediction hits of a fourth -- as ONE row of scalars per
// workgroup, from ONE encoder output (training_cvs.py:43-144: evaluate_loss x 2, recon, classifier / pred_inputs).
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid):
//   E0  labels, loc / scale, the four noise rows (Philox in-kernel or explicit [4, B, L]); conditional priors; z1 (main), z2 (auxiliary),
//       z3 (recon: posterior or prior draw), z4 (label prediction); log q - log p of z1
//   E1  time-invariant part of the hidden layer and the initial state of BOTH solves (z1, z3)
//   E2  step coefficients x' = A x + b of every grid step (f = a(t, z) - d(t, z) x: tests/kernel_math.py step_coeffs), thread <-> step,
//       solve z1 on waves 0-1 and solve z3 on waves 2-3; forward only: no adjoint, no gradient rows
//   E3  forward affine scan: one (solve, state component) per wave pass, a chunk of steps per lane, Kogge-Stone over the lanes' maps
//   E4  thread <-> time point: decoder heads + ALD / Gaussian likelihood of the z1 trajectory (likelihood scales from the fold launch's
//       table) and |centre head - observation| of the z3 trajectory, the observation read once for both
//   E5  label heads, a half-wave per (head, use): auxiliary loss terms on z2, decision + hit test on z4, the main loss's label terms on z1
//       (proc family)
// Every sum runs in a fixed order (lane trees, wave order, the reduction launch in row order): bitwise reproducible, no atomics.
#include "slode_common.h"

namespace {

constexpr int EV_NT = 256;
constexpr float EV_HL2PI = 0.91893853320467274178f;

struct EvalK {
  int B, T, C, L, S, H, nu, n_groups, n_aux, U, R, method, gauss, aux_in_main, is_post, Q;
  float aux_mult, tau[3];
  slode_group grp[SLODE_MAX_GROUPS];
  slode_aux aux[SLODE_MAX_AUX];
  int ploc_w[SLODE_MAX_GROUPS], ploc_b[SLODE_MAX_GROUPS], pls_w[SLODE_MAX_GROUPS], pls_b[SLODE_MAX_GROUPS];
  int init_w1, init_b1, init_w2, init_b2, dyn_wh, dyn_bh, dyn_wg, dyn_bg, dyn_wd, dyn_bd, head[SLODE_MAX_HEADS];
  int aux_w1[SLODE_MAX_AUX], aux_b1[SLODE_MAX_AUX], aux_w2[SLODE_MAX_AUX], aux_b2[SLODE_MAX_AUX], aux_c[SLODE_MAX_AUX];
  const float *params, *times, *stage_t, *obs;
  long long sb, sc, st;
  const float *loc, *scale, *eps, *u, *sigtab;
  float* part;   // [grid][SLODE_EVAL_SLOTS]
  RngK rng;
  LabelSrc lab;
};

// a(t, z), d(t, z) of one stage time: sigmoid heads over relu(w_t t + u) (models/blackbox_ode.py:97-109); the weights are uniform operands
template <int SM>
__device__ __forceinline__ void eval_ad(const EvalK& k, const float* __restrict__ par, const float* s_uh, float t, int S, float (&a)[SM], float (&d)[SM]) {
#pragma unroll
  for (int s = 0; s < SM; ++s) { a[s] = s < S ? par[k.dyn_bg + s] : 0.f; d[s] = s < S ? par[k.dyn_bd + s] : 0.f; }
  const int H = k.H, WS = 1 + k.L;
  for (int j = 0; j < H; ++j) {
    const float hj = fmaxf(fmaf(par[k.dyn_wh + j * WS], t, s_uh[j]), 0.f);
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (s < S) { a[s] = fmaf(par[k.dyn_wg + s * H + j], hj, a[s]); d[s] = fmaf(par[k.dyn_wd + s * H + j], hj, d[s]); }
  }
#pragma unroll
  for (int s = 0; s < SM; ++s) { a[s] = sigmoidf_fast(a[s]); d[s] = sigmoidf_fast(d[s]); }
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(EV_NT) eval_stats_kernel(const EvalK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ float s_ab[];   // A[2][T-1][S] (overwritten by x[.][n+1][.] in the scan) | b[2][T-1][S]
  __shared__ float s_z[4 * SLODE_MAX_L], s_loc[SLODE_MAX_L], s_sc[SLODE_MAX_L], s_u[SLODE_MAX_NU];
  __shared__ float s_uh[2 * SLODE_MAX_H], s_h0[2 * SLODE_MAX_H], s_x0[2 * SLODE_MAX_S], s_item[16], s_red[EV_NT / 64];
  const float* __restrict__ par = k.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = tid >> 5, j32 = tid & 31;
  const int T = k.T, L = k.L, S = SC ? SC : k.S, H = k.H, C = k.C, U = k.U, R = k.R, NS = T - 1;
  float* s_A = s_ab;
  float* s_B = s_ab + 2 * NS * S;
  const int n_items = k.n_aux * (2 + (k.aux_in_main ? 1 : 0));
  float loss_main = 0.f, l1_acc = 0.f, item_acc = 0.f;
  int count = 0;

  for (int b = blockIdx.x; b < k.B; b += gridDim.x) {
    ++count;
    // ---- E0 ----
    if (tid < k.nu) s_u[tid] = slode_label_at(k.lab, k.u, k.nu, b, tid);
    __syncthreads();   // (also: the previous trajectory's readers of s_z / s_x0 / s_ab / s_item are done)
    if (tid < L) {
      const int l = tid;
      const float loc = k.loc[(long long)b * L + l], sc = k.scale[(long long)b * L + l];
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
      const float e0 = slode_eps_at(k.rng, k.eps, b, L, l, 0, k.B), e1 = slode_eps_at(k.rng, k.eps, b, L, l, 1, k.B);
      const float e2 = slode_eps_at(k.rng, k.eps, b, L, l, 2, k.B), e3 = slode_eps_at(k.rng, k.eps, b, L, l, 3, k.B);
      const float z = fmaf(sc, e0, loc);
      const float ips = expf(-pls), dz = (z - pl) * ips, zq = (z - loc) / sc;
      loss_main += (-logf(sc) - EV_HL2PI - 0.5f * zq * zq) - (-pls - EV_HL2PI - 0.5f * dz * dz);   // log q - log p
      s_z[l] = z;
      s_z[SLODE_MAX_L + l] = fmaf(sc, e1, loc);
      s_z[2 * SLODE_MAX_L + l] = k.is_post ? fmaf(sc, e2, loc) : fmaf(expf(pls), e2, pl);
      s_z[3 * SLODE_MAX_L + l] = fmaf(sc, e3, loc);
      s_loc[l] = loc; s_sc[l] = sc;
    }
    __syncthreads();
    // ---- E1: u = W_z z + b_h and the init net's hidden layer, for z1 (q = 0) and z3 (q = 1) ----
    if (tid < 4 * H) {
      const int q = tid / (2 * H), r = tid - q * 2 * H, which = r / H, j = r - which * H;
      const float* zz = s_z + (q ? 2 * SLODE_MAX_L : 0);
      if (which == 0) {
        float v = par[k.dyn_bh + j];
        for (int l = 0; l < L; ++l) v = fmaf(par[k.dyn_wh + j * (1 + L) + 1 + l], zz[l], v);
        s_uh[q * SLODE_MAX_H + j] = v;
      } else {
        float v = par[k.init_b1 + j];
        for (int l = 0; l < L; ++l) v = fmaf(par[k.init_w1 + j * L + l], zz[l], v);
        s_h0[q * SLODE_MAX_H + j] = fmaxf(v, 0.f);
      }
    }
    __syncthreads();
    if (tid < 2 * S) {
      const int q = tid / S, s = tid - q * S;
      float o = par[k.init_b2 + s];
      for (int j = 0; j < H; ++j) o = fmaf(par[k.init_w2 + s * H + j], s_h0[q * SLODE_MAX_H + j], o);
      s_x0[q * SLODE_MAX_S + s] = sigmoidf_fast(o);
    }
    // ---- E2: step coefficients; waves 0-1: solve z1, waves 2-3: solve z3 ----
    {
      const int q = wave >> 1;
      const float* uh = s_uh + q * SLODE_MAX_H;
      for (int n = tid & 127; n < NS; n += 128) {
        const float h = k.times[n + 1] - k.times[n];
        float a[SM], d[SM], A[SM], bb[SM];
        eval_ad<SM>(k, par, uh, k.stage_t[n * R], S, a, d);
        if (k.method == SLODE_EULER) {
#pragma unroll
          for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s]; bb[s] = h * a[s]; }
        } else if (k.method == SLODE_MIDPOINT) {
          float m[SM], c[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) { m[s] = 1.f - 0.5f * h * d[s]; c[s] = 0.5f * h * a[s]; }
          eval_ad<SM>(k, par, uh, k.stage_t[n * R + 1], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) { A[s] = 1.f - h * d[s] * m[s]; bb[s] = h * (a[s] - d[s] * c[s]); }
        } else {   // torchdiffeq's rk4: the 3/8 rule
          const float third = 1.0f / 3.0f, h3 = h * third;
          float p1[SM], q1[SM], p2[SM], q2[SM], c[SM], m[SM];
#pragma unroll
          for (int s = 0; s < SM; ++s) { p1[s] = a[s]; q1[s] = -d[s]; c[s] = h3 * p1[s]; m[s] = 1.f + h3 * q1[s]; }
          eval_ad<SM>(k, par, uh, k.stage_t[n * R + 1], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            p2[s] = a[s] - d[s] * c[s]; q2[s] = -d[s] * m[s];
            c[s] = h * (p2[s] - p1[s] * third); m[s] = 1.f + h * (q2[s] - q1[s] * third);
          }
          eval_ad<SM>(k, par, uh, k.stage_t[n * R + 2], S, a, d);
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            const float p3 = a[s] - d[s] * c[s], q3 = -d[s] * m[s];
            c[s] = h * (p1[s] - p2[s] + p3); m[s] = 1.f + h * (q1[s] - q2[s] + q3);
            A[s] = q1[s] + 3.f * (q2[s] + q3); bb[s] = p1[s] + 3.f * (p2[s] + p3);   // (partial sums: q4 / p4 follow)
          }
          eval_ad<SM>(k, par, uh, k.stage_t[n * R + 3], S, a, d);
          const float G = h * 0.125f;
#pragma unroll
          for (int s = 0; s < SM; ++s) {
            const float p4 = a[s] - d[s] * c[s], q4 = -d[s] * m[s];
            A[s] = 1.f + G * (A[s] + q4); bb[s] = G * (bb[s] + p4);
          }
        }
#pragma unroll
        for (int s = 0; s < SM; ++s)
          if (s < S) { s_A[(q * NS + n) * S + s] = A[s]; s_B[(q * NS + n) * S + s] = bb[s]; }
      }
    }
    __syncthreads();
    // ---- E3: forward affine scan, in place: x[q][n + 1][s] takes the slot of A[q][n][s] ----
    {
      const int q = wave >> 1, chunk = (NS + 63) / 64, n0 = min(lane * chunk, NS), n1 = min(n0 + chunk, NS);
      for (int s = wave & 1; s < S; s += 2) {
        float* pa = s_A + (q * NS) * S + s;
        const float* pb = s_B + (q * NS) * S + s;
        float Ac = 1.f, bc = 0.f;   // the lane's chunk as one map
        for (int n = n0; n < n1; ++n) { const float An = pa[n * S]; bc = fmaf(An, bc, pb[n * S]); Ac *= An; }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {   // inclusive scan of the maps over the lanes (later map o earlier map)
          const float Ap = __shfl_up(Ac, off, 64), bp = __shfl_up(bc, off, 64);
          if (lane >= off) { bc = fmaf(Ac, bp, bc); Ac *= Ap; }
        }
        float Ae = __shfl_up(Ac, 1, 64), be = __shfl_up(bc, 1, 64);
        if (lane == 0) { Ae = 1.f; be = 0.f; }
        float x = fmaf(Ae, s_x0[q * SLODE_MAX_S + s], be);
        for (int n = n0; n < n1; ++n) { x = fmaf(pa[n * S], x, pb[n * S]); pa[n * S] = x; }
      }
    }
    __syncthreads();
    // ---- E4: heads + likelihood of the z1 trajectory, |centre - observation| of the z3 trajectory ----
    {
      const int CT = C * T;
      for (int t = tid; t < T; t += EV_NT) {
        float x1[SM], x3[SM];
#pragma unroll
        for (int s = 0; s < SM; ++s) {
          x1[s] = s < S ? (t == 0 ? s_x0[s] : s_A[(t - 1) * S + s]) : 0.f;
          x3[s] = s < S ? (t == 0 ? s_x0[SLODE_MAX_S + s] : s_A[(NS + t - 1) * S + s]) : 0.f;
        }
        float ll = 0.f, l1 = 0.f;
        for (int c = 0; c < C; ++c) {
          const float obv = k.obs[(long long)b * k.sb + c * k.sc + t * k.st];
          const float inv = k.sigtab[CT + c * T + t], lg = k.sigtab[2 * CT + c * T + t];
          for (int q = 0; q < k.Q; ++q) {
            float mu = 0.f;
#pragma unroll
            for (int s = 0; s < SM; ++s) if (s < S) mu = fmaf(par[k.head[q] + c * S + s], x1[s], mu);
            const float r = obv - mu;
            if (k.gauss) ll += -lg - EV_HL2PI - 0.5f * r * r * inv * inv;
            else ll += ((obv >= mu) ? k.tau[q] : 1.f - k.tau[q]) * (-lg - fabsf(r) * inv);
          }
          float mu3 = 0.f;
#pragma unroll
          for (int s = 0; s < SM; ++s) if (s < S) mu3 = fmaf(par[k.head[0] + c * S + s], x3[s], mu3);
          l1 += fabsf(mu3 - obv);
        }
        loss_main -= ll;
        l1_acc += l1;
      }
    }
    // ---- E5: label heads; half-wave = (use, head), lane = hidden unit ----
    for (int it0 = 0; it0 < n_items; it0 += EV_NT / 32) {
      const int item = it0 + hw;
      const bool on = item < n_items;
      const int itc = on ? item : 0, use = itc / k.n_aux, a = itc - use * k.n_aux;   // use 0: auxiliary loss (z2), 1: prediction (z4), 2: main loss (z1)
      const slode_aux ax = k.aux[a];
      const int zd = ax.z_dim, ud = ax.u_dim;
      const float* zz = s_z + (use == 0 ? 1 : (use == 1 ? 3 : 0)) * SLODE_MAX_L + ax.z_off;
      const bool unit_on = j32 < U;
      const int jj = min(j32, U - 1);
      float pre = par[k.aux_b1[a] + jj];
      for (int l = 0; l < zd; ++l) pre = fmaf(par[k.aux_w1[a] + jj * zd + l], zz[l], pre);
      const float hv = unit_on ? softplusf(pre) : 0.f;
      float lg[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) {   // (every lane of the wave takes part in every sum: columns beyond u_dim add zeros)
        const float w = (q < ud) ? par[k.aux_w2[a] + min(q, ud - 1) * U + jj] : 0.f;
        lg[q] = half_wave_sum(w * hv) + par[k.aux_b2[a] + min(q, ud - 1)];
      }
      // -log N(z_g; loc, scale) of the head's dims (auxiliary loss: the group latents are sampled in the model)
      float nl = 0.f;
      if (j32 < zd) {
        const float loc = s_loc[ax.z_off + j32], sc = s_sc[ax.z_off + j32], zq = (zz[j32] - loc) / sc;
        nl = logf(sc) + EV_HL2PI + 0.5f * zq * zq;
      }
      nl = half_wave_sum(nl);
      float lp = 0.f;
      bool hit = true;
      if (ax.kind == SLODE_AUX_SOFTMAX) {
        float mx = -3.0e38f, se = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) mx = fmaxf(mx, lg[q]);
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) se += expf(lg[q] - mx);
        const float lse = mx + logf(se);
        int arg = 0;
        float best = -1.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) {
          lp = fmaf(s_u[ax.u_off + q], lg[q] - lse, lp);
          const float pq = expf(lg[q] - mx) / se;   // the class probability slode_label_heads writes
          if (pq > best) { best = pq; arg = q; }    // lowest index on a tie (torch.argmax)
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) hit = hit && fabsf((q == arg ? 1.f : 0.f) - s_u[ax.u_off + q]) < 0.5f;
      } else if (ax.kind == SLODE_AUX_SIGMOID) {
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) {
          const float o = lg[q], y = s_u[ax.u_off + q];
          const float sp_pos = (o > 0.f ? o : 0.f) + log1pf(expf(-fabsf(o)));
          lp += y * (o - sp_pos) + (1.f - y) * (-sp_pos);
          const float pr = 1.f / (1.f + expf(-o));
          hit = hit && fabsf((pr > 0.5f ? 1.f : 0.f) - y) < 0.5f;
        }
      } else {   // EXPEXP: Laplace(exp(head 0), softplus(constant_std_*)); the prediction is the location
        const float bsc = softplusf(par[k.aux_c[a]]), ib = 1.f / bsc;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) {
          const float lc = expf(lg[q]), y = s_u[ax.u_off + q];
          lp += -logf(2.f * bsc) - fabsf(y - lc) * ib;
          hit = hit && fabsf(lc - y) < 0.5f;
        }
      }
      if (on && j32 == 0) s_item[item] = use == 0 ? nl - k.aux_mult * lp : (use == 1 ? (hit ? 1.f : 0.f) : -k.aux_mult * lp);
    }
    __syncthreads();
    if (tid < n_items) item_acc += s_item[tid];
  }

  // ---- the workgroup's row: [main | auxiliary | L1 | hits per head | trajectories] ----
  const float v0 = block_sum(loss_main, s_red);
  const float v2 = block_sum(l1_acc, s_red);
  __syncthreads();
  if (tid < n_items) s_item[tid] = item_acc;
  __syncthreads();
  if (tid == 0) {
    float* row = k.part + (long long)blockIdx.x * SLODE_EVAL_SLOTS;
    float main = v0, auxl = 0.f;
    for (int a = 0; a < k.n_aux; ++a) {
      auxl += s_item[a];
      if (k.aux_in_main) main += s_item[2 * k.n_aux + a];
    }
    row[0] = main; row[1] = auxl; row[2] = v2;
    for (int a = 0; a < SLODE_MAX_AUX; ++a) row[3 + a] = a < k.n_aux ? s_item[k.n_aux + a] : 0.f;
    row[SLODE_EVAL_SLOTS - 1] = (float)count;
  }
}

// out[slot] = sum over the n partial rows, fixed order: thread i takes rows i, i + 256, ...; then a fixed tree (fp64: the counts stay exact)
__global__ void __launch_bounds__(256) eval_reduce_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ double s_s[256];
  const int slot = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  for (int w = tid; w < n; w += 256) acc += (double)part[(long long)w * SLODE_EVAL_SLOTS + slot];
  s_s[tid] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) s_s[tid] += s_s[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[slot] = (float)s_s[0];
}

}  // namespace

size_t slode_eval_lds_bytes(const slode_shape& s) { return (size_t)4 * (s.T - 1) * s.S * sizeof(float); }

hipError_t slode_launch_eval(const EvalLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  EvalK k{};
  k.B = s.B; k.T = s.T; k.C = s.C; k.L = s.L; k.S = s.S; k.H = s.H; k.nu = s.n_u; k.n_groups = s.n_groups; k.n_aux = s.n_aux; k.U = s.U;
  k.method = s.method; k.R = s.method == SLODE_EULER ? 1 : (s.method == SLODE_MIDPOINT ? 2 : 3);
  k.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; k.Q = k.gauss ? 1 : 3; k.aux_in_main = s.aux_in_main && s.n_aux > 0 ? 1 : 0; k.is_post = a.is_post;
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
  k.params = a.params; k.times = a.times; k.stage_t = a.stage_t; k.obs = a.obs; k.sb = a.sb; k.sc = a.sc; k.st = a.st;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u; k.sigtab = a.sigtab; k.part = a.part; k.rng = a.rng; k.lab = a.lab;
  const size_t lds = slode_eval_lds_bytes(s);
  if (lds + 4096 > 160 * 1024) return hipErrorInvalidValue;
#define SLODE_EVAL_GO(SC)                                                                                                               \
  do {                                                                                                                                  \
    if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)eval_stats_kernel<SC>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    SLODE_LAUNCH("eval_stats", eval_stats_kernel<SC>, dim3(a.grid), dim3(EV_NT), lds, stream, k);                                        \
  } while (0)
  if (!a.force_generic && s.S == 5) SLODE_EVAL_GO(5);
  else if (!a.force_generic && s.S == 8) SLODE_EVAL_GO(8);
  else SLODE_EVAL_GO(0);
#undef SLODE_EVAL_GO
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  SLODE_LAUNCH("eval_reduce", eval_reduce_kernel, dim3(SLODE_EVAL_SLOTS), dim3(256), 0, stream, a.part, a.grid, a.out);
  return hipGetLastError();
}
