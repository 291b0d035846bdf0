// Fused statistics pass (slode_eval_stats): what one batch of the reference's per-epoch statistics needs -- the -ELBO of the main loss, the
// auxiliary loss, the reconstruction L1 of one more latent draw and the label-prediction hits of a fourth -- as ONE row of scalars per
// workgroup, from ONE encoder output (training_cvs.py:43-144: evaluate_loss x 2, recon, classifier / pred_inputs).
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid):
//   E0  labels, loc / scale, the four noise rows (Philox in-kernel or explicit [4, B, L]); conditional priors; z1 (main), z2 (auxiliary),
//       z3 (recon: posterior or prior draw), z4 (label prediction); log q - log p of z1
//   E1  time-invariant part of the hidden layer and the initial state of BOTH solves (z1, z3)
//   E2  step coefficients x' = A x + b of every grid step (fwd_step_table, slode_forward.h), thread <-> step, the weights as uniform
//       operands from global memory; solve z1 on waves 0-1 and solve z3 on waves 2-3; forward only: no adjoint, no gradient rows
//   E3  forward affine scan (fwd_scan, slode_forward.h): one (solve, state component) per wave pass
//   E4  thread <-> time point: decoder heads + ALD / Gaussian likelihood of the z1 trajectory (likelihood scales from the fold launch's
//       table) and |centre head - observation| of the z3 trajectory, the observation read once for both
//   E5  label heads (logits: fwd_label_logits, slode_forward.h), a half-wave per (head, use): auxiliary loss terms on z2, decision + hit test on z4, the main loss's label terms on z1
//       (proc family)
// Every sum runs in a fixed order (lane trees, wave order, the reduction launch in row order): bitwise reproducible, no atomics.
#include "slode_forward.h"

namespace {

constexpr int EV_NT = FWD_NT;
constexpr float EV_HL2PI = FWD_HL2PI;

struct EvalK {
  FwdK f;
  PriorK pr;
  LabelHeadK lh;
  int gauss, aux_in_main, is_post;
  float tau[3];
  const float* obs;
  long long sb, sc, st;
  const float *loc, *scale, *eps, *u, *sigtab;
  float* part;   // [grid][SLODE_EVAL_SLOTS]
  RngK rng;
  LabelSrc lab;
};

// a(t, z), d(t, z) of one stage time: sigmoid heads over relu(w_t t + u) (models/blackbox_ode.py:97-109); the weights are uniform operands
template <int SM>
__device__ __forceinline__ void eval_ad(const FwdK& k, const float* __restrict__ par, const float* s_uh, float t, int S, float (&a)[SM], float (&d)[SM]) {
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
  const FwdK& f = k.f;
  const float* __restrict__ par = f.params;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = tid >> 5, j32 = tid & 31;
  const int T = f.T, L = f.L, S = SC ? SC : f.S, H = f.H, C = f.C, NS = T - 1, n_aux = k.lh.n_aux;
  float* s_A = s_ab;
  float* s_B = s_ab + 2 * NS * S;
  const int n_items = n_aux * (2 + (k.aux_in_main ? 1 : 0));
  float loss_main = 0.f, l1_acc = 0.f, item_acc = 0.f;
  int count = 0;

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    ++count;
    // ---- E0 ----
    if (tid < k.pr.nu) s_u[tid] = slode_label_at(k.lab, k.u, k.pr.nu, b, tid);
    __syncthreads();   // (also: the previous trajectory's readers of s_z / s_x0 / s_ab / s_item are done)
    if (tid < L) {
      const int l = tid;
      const float loc = k.loc[(long long)b * L + l], sc = k.scale[(long long)b * L + l];
      float pl, pls;
      fwd_prior_at(k.pr, par, s_u, l, pl, pls);
      const float e0 = slode_eps_at(k.rng, k.eps, b, L, l, 0, f.B), e1 = slode_eps_at(k.rng, k.eps, b, L, l, 1, f.B);
      const float e2 = slode_eps_at(k.rng, k.eps, b, L, l, 2, f.B), e3 = slode_eps_at(k.rng, k.eps, b, L, l, 3, f.B);
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
        float v = par[f.dyn_bh + j];
        for (int l = 0; l < L; ++l) v = fmaf(par[f.dyn_wh + j * (1 + L) + 1 + l], zz[l], v);
        s_uh[q * SLODE_MAX_H + j] = v;
      } else {
        float v = par[f.init_b1 + j];
        for (int l = 0; l < L; ++l) v = fmaf(par[f.init_w1 + j * L + l], zz[l], v);
        s_h0[q * SLODE_MAX_H + j] = fmaxf(v, 0.f);
      }
    }
    __syncthreads();
    if (tid < 2 * S) {
      const int q = tid / S, s = tid - q * S;
      float o = par[f.init_b2 + s];
      for (int j = 0; j < H; ++j) o = fmaf(par[f.init_w2 + s * H + j], s_h0[q * SLODE_MAX_H + j], o);
      s_x0[q * SLODE_MAX_S + s] = sigmoidf_fast(o);
    }
    // ---- E2: step coefficients; waves 0-1: solve z1, waves 2-3: solve z3 ----
    {
      const int q = wave >> 1;
      const float* uh = s_uh + q * SLODE_MAX_H;
      fwd_step_table<SM>(f, S, 0, NS, tid & 127, 128, s_A + q * NS * S, s_B + q * NS * S,
                         [&](float t, float (&a)[SM], float (&d)[SM]) { eval_ad<SM>(f, par, uh, t, S, a, d); });
    }
    __syncthreads();
    // ---- E3: forward affine scan, in place: x[q][n + 1][s] takes the slot of A[q][n][s] ----
    {
      const int q = wave >> 1;
      fwd_scan(s_A + q * NS * S, s_B + q * NS * S, s_x0 + q * SLODE_MAX_S, S, NS, lane, wave & 1, 2);
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
          for (int q = 0; q < f.Q; ++q) {
            float mu = 0.f;
#pragma unroll
            for (int s = 0; s < SM; ++s) if (s < S) mu = fmaf(par[f.head[q] + c * S + s], x1[s], mu);
            const float r = obv - mu;
            if (k.gauss) ll += -lg - EV_HL2PI - 0.5f * r * r * inv * inv;
            else ll += ((obv >= mu) ? k.tau[q] : 1.f - k.tau[q]) * (-lg - fabsf(r) * inv);
          }
          float mu3 = 0.f;
#pragma unroll
          for (int s = 0; s < SM; ++s) if (s < S) mu3 = fmaf(par[f.head[0] + c * S + s], x3[s], mu3);
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
      const int itc = on ? item : 0, use = itc / n_aux, a = itc - use * n_aux;   // use 0: auxiliary loss (z2), 1: prediction (z4), 2: main loss (z1)
      const slode_aux ax = k.lh.aux[a];
      const int zd = ax.z_dim, ud = ax.u_dim;
      const float* zz = s_z + (use == 0 ? 1 : (use == 1 ? 3 : 0)) * SLODE_MAX_L + ax.z_off;
      float lg[8];
      fwd_label_logits(k.lh, par, a, zz, j32, lg);
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
        const float bsc = softplusf(par[k.lh.aux_c[a]]), ib = 1.f / bsc;
#pragma unroll
        for (int q = 0; q < 8; ++q) if (q < ud) {
          const float lc = expf(lg[q]), y = s_u[ax.u_off + q];
          lp += -logf(2.f * bsc) - fabsf(y - lc) * ib;
          hit = hit && fabsf(lc - y) < 0.5f;
        }
      }
      if (on && j32 == 0) s_item[item] = use == 0 ? nl - k.lh.aux_mult * lp : (use == 1 ? (hit ? 1.f : 0.f) : -k.lh.aux_mult * lp);
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
    for (int a = 0; a < n_aux; ++a) {
      auxl += s_item[a];
      if (k.aux_in_main) main += s_item[2 * n_aux + a];
    }
    row[0] = main; row[1] = auxl; row[2] = v2;
    for (int a = 0; a < SLODE_MAX_AUX; ++a) row[3 + a] = a < n_aux ? s_item[n_aux + a] : 0.f;
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
  fwd_fill(k.f, s, lay, a.params, a.times, a.stage_t); fwd_fill(k.pr, s, lay); fwd_fill(k.lh, s, lay);
  k.gauss = s.likelihood == SLODE_GAUSS ? 1 : 0; k.aux_in_main = s.aux_in_main && s.n_aux > 0 ? 1 : 0; k.is_post = a.is_post;
  k.tau[0] = 0.5f; k.tau[1] = 0.5f + s.quantile_diff; k.tau[2] = 0.5f - s.quantile_diff;
  k.obs = a.obs; k.sb = a.sb; k.sc = a.sc; k.st = a.st;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u; k.sigtab = a.sigtab; k.part = a.part; k.rng = a.rng; k.lab = a.lab;
  const size_t lds = slode_eval_lds_bytes(s);
  if (lds + 4096 > 160 * 1024) return hipErrorInvalidValue;
  fwd_dispatch(s, a.force_generic, [&](auto sc) { fwd_launch("eval_stats", eval_stats_kernel<decltype(sc)::value>, a.grid, lds, stream, k); });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  SLODE_LAUNCH("eval_reduce", eval_reduce_kernel, dim3(SLODE_EVAL_SLOTS), dim3(256), 0, stream, a.part, a.grid, a.out);
  return hipGetLastError();
}
