// The fixed-grid forward pass and the draw loop the eval-side kernels share (eval_kernel.hip, recon_moments_kernel.hip,
// intervene_moments_kernel.hip, forecast_moments_kernel.hip, cohort_moments_kernel.hip, calibration_kernel.hip; the five whole-curve kernels
// attribution_kernel.hip, curve_summary_kernel.hip, recon_quantiles_kernel.hip, mechanism_moments_kernel.hip, joint_band_kernel.hip; and,
// through traj_terms.h, traj_bounds_kernel.hip, pointwise_kernel.hip, refine_kernel.hip; no other translation unit includes this header):
// each phase ONCE --
//   kernel arguments   FwdK (dims, solver, the init / dynamics / head offsets), PriorK (conditional prior nets), LabelHeadK (label heads),
//                      DrawsK (FwdK, PriorK and where the draws of a call come from: recon, cohort, calibration) and the host functions that
//                      fill them from slode_shape / slode_layout / DrawsLaunch
//   prior nets         fwd_prior_at: loc / log scale of one latent dim from the staged labels
//   step coefficients  fwd_step_coeffs (fixed_step.h, beside the training kernel's step_fwd): x' = A x + b of one grid step for euler /
//                      midpoint / rk4, the a, d evaluator passed in;
//                      fwd_step_table: thread <-> step, the table of a step range [n_lo, n_hi) of the grid (a whole solve: [0, T - 1))
//   scan               fwd_scan: forward affine scan, one state component per wave pass
//   label heads        fwd_label_logits: hidden layer and logits of one head on a half-wave
//   staged weights     (every kernel but eval_stats) FWD_ROW, FwdLds / FwdSm, fwd_stage_weights, fwd_init_state, fwd_ad, fwd_step_table_staged:
//                      the weights every draw reuses live in the LDS; the a, d evaluator reads one 16-byte-aligned row per hidden unit
//   the draw loop       M1 fwd_draw_source: loc | scale of a trajectory, posterior or conditional prior, into the LDS pieces of
//                      fwd_lds_loc_sc; M2 fwd_draw_z: z of draw k; M3-M5 fwd_solve: one solve of a step range from a given initial state;
//                      M6 fwd_state_at, fwd_head_value: the state of a time point, one head value; the shifted moment triple [v0 | s1 | s2]:
//                      fwd_moment_add, fwd_moment_store (M7), fwd_moment_store_pinned (M7 of the kernels whose moments the tests restate
//                      bit for bit in numpy)
//   launch             fwd_generic, fwd_dispatch over the compile-time state dim {5, 8, 0}, fwd_launch
// Every routine keeps the operation order of the kernels it came from: results are bitwise those of the separate copies.
#pragma once
#include <type_traits>
#include "slode_common.h"
#include "fixed_step.h"

namespace {   // (internal linkage: every including translation unit has its own copy, as before)

constexpr int FWD_NT = 256;   // threads of a workgroup: four waves
constexpr float FWD_HL2PI = 0.91893853320467274178f;
#define FWD_ROW(SM) ((2 + 2 * (SM) + 3) & ~3)   // floats of one hidden unit's LDS row: w_t | u_j | W_g[0..SM) | W_d[0..SM)

// ---- kernel-argument parts ----------------------------------------------------------------------------------
struct FwdK {
  int B, T, C, L, S, H, R, method, Q;
  int init_w1, init_b1, init_w2, init_b2, dyn_wh, dyn_bh, dyn_wg, dyn_bg, dyn_wd, dyn_bd, head[SLODE_MAX_HEADS];
  const float *params, *times, *stage_t;
};
struct PriorK {
  int nu, n_groups;
  slode_group grp[SLODE_MAX_GROUPS];
  int ploc_w[SLODE_MAX_GROUPS], ploc_b[SLODE_MAX_GROUPS], pls_w[SLODE_MAX_GROUPS], pls_b[SLODE_MAX_GROUPS];
};
struct LabelHeadK {
  int n_aux, U;
  float aux_mult;
  slode_aux aux[SLODE_MAX_AUX];
  int aux_w1[SLODE_MAX_AUX], aux_b1[SLODE_MAX_AUX], aux_w2[SLODE_MAX_AUX], aux_b2[SLODE_MAX_AUX], aux_c[SLODE_MAX_AUX];
};
// a call that walks ns draws per trajectory from one source: the posterior (loc / scale of the encoder launch) or the conditional prior
struct DrawsK {
  FwdK f;
  PriorK pr;
  int is_post, ns;
  const float *loc, *scale, *eps, *u;
  RngK rng;
  LabelSrc lab;
};

inline void fwd_fill(FwdK& k, const slode_shape& s, const slode_layout& lay, const float* params, const float* times, const float* stage_t) {
  k.B = s.B; k.T = s.T; k.C = s.C; k.L = s.L; k.S = s.S; k.H = s.H;
  k.method = s.method; k.R = fixed_step_times(s.method);
  k.Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  k.init_w1 = lay.init_w1; k.init_b1 = lay.init_b1; k.init_w2 = lay.init_w2; k.init_b2 = lay.init_b2;
  k.dyn_wh = lay.dyn_wh; k.dyn_bh = lay.dyn_bh; k.dyn_wg = lay.dyn_wg; k.dyn_bg = lay.dyn_bg; k.dyn_wd = lay.dyn_wd; k.dyn_bd = lay.dyn_bd;
  for (int q = 0; q < SLODE_MAX_HEADS; ++q) k.head[q] = lay.head_w[q];
  k.params = params; k.times = times; k.stage_t = stage_t;
}
inline void fwd_fill(PriorK& k, const slode_shape& s, const slode_layout& lay) {
  k.nu = s.n_u; k.n_groups = s.n_groups;
  for (int g = 0; g < SLODE_MAX_GROUPS; ++g) {
    k.grp[g] = s.groups[g]; k.ploc_w[g] = lay.ploc_w[g]; k.ploc_b[g] = lay.ploc_b[g]; k.pls_w[g] = lay.pls_w[g]; k.pls_b[g] = lay.pls_b[g];
  }
}
inline void fwd_fill(LabelHeadK& k, const slode_shape& s, const slode_layout& lay) {
  k.n_aux = s.n_aux; k.U = s.U; k.aux_mult = s.aux_mult;
  for (int q = 0; q < SLODE_MAX_AUX; ++q) {
    k.aux[q] = s.aux[q]; k.aux_w1[q] = lay.aux_w1[q]; k.aux_b1[q] = lay.aux_b1[q]; k.aux_w2[q] = lay.aux_w2[q]; k.aux_b2[q] = lay.aux_b2[q];
    k.aux_c[q] = lay.aux_c[q];
  }
}
inline void fwd_fill(DrawsK& k, const DrawsLaunch& a) {
  fwd_fill(k.f, a.s, a.lay, a.params, a.times, a.stage_t); fwd_fill(k.pr, a.s, a.lay);
  k.is_post = a.is_post; k.ns = a.num_samples;
  k.loc = a.loc; k.scale = a.scale; k.eps = a.eps; k.u = a.u; k.rng = a.rng; k.lab = a.lab;
}

// ---- conditional prior nets -----------------------------------------------------------------------------------
// loc pl and log scale pls of latent dim l under its group's prior nets on the staged labels s_u; false (pl = pls = 0) when l lies in no
// group whose bit is set in mask (intervene: the intervened groups; everyone else: all)
__device__ __forceinline__ bool fwd_prior_at(const PriorK& k, const float* __restrict__ par, const float* s_u, int l, float& pl, float& pls,
                                             int mask = -1) {
  bool found = false;
  pl = 0.f; pls = 0.f;
  for (int g = 0; g < k.n_groups; ++g) {
    const slode_group gr = k.grp[g];
    if (((mask >> g) & 1) && l >= gr.z_off && l < gr.z_off + gr.z_dim) {
      const int ll = l - gr.z_off;
      pl = par[k.ploc_b[g] + ll]; pls = par[k.pls_b[g] + ll];
      for (int q = 0; q < gr.u_dim; ++q) {
        const float uv = s_u[gr.u_off + q];
        pl = fmaf(par[k.ploc_w[g] + ll * gr.u_dim + q], uv, pl);
        pls = fmaf(par[k.pls_w[g] + ll * gr.u_dim + q], uv, pls);
      }
      found = true;
    }
  }
  return found;
}

// ---- step coefficients ------------------------------------------------------------------------------------------
// the step table of the steps [n_lo, n_hi) of the grid k.times / k.stage_t (a whole solve: n_lo = 0, n_hi = T - 1), thread <-> step: step
// n_lo + i into pa[i][s] / pb[i][s], i = i_first, i_first + i_stride, ...
template <int SM, class AD>
__device__ __forceinline__ void fwd_step_table(const FwdK& k, int S, int n_lo, int n_hi, int i_first, int i_stride, float* pa, float* pb,
                                               const AD& ad) {
  for (int i = i_first; i < n_hi - n_lo; i += i_stride) {
    const long long n = (long long)n_lo + i;
    float A[SM], bb[SM];
    fwd_step_coeffs<SM>(k.method, k.times[n + 1] - k.times[n], k.stage_t + n * k.R, ad, A, bb);
#pragma unroll
    for (int s = 0; s < SM; ++s)
      if (s < S) { pa[i * S + s] = A[s]; pb[i * S + s] = bb[s]; }
  }
}

// ---- forward affine scan ---------------------------------------------------------------------------------------
// In place: x[n + 1][s] takes the slot of A[n][s] (pa, pb: [NS][S]; x0: [S]).  One state component per wave pass -- s_first, s_first +
// s_stride, ... -- a chunk of steps per lane, Kogge-Stone over the lanes' maps.  Call with whole waves.
__device__ __forceinline__ void fwd_scan(float* pa, const float* pb, const float* x0, int S, int NS, int lane, int s_first, int s_stride) {
  const int chunk = (NS + 63) / 64, n0 = min(lane * chunk, NS), n1 = min(n0 + chunk, NS);
  for (int s = s_first; s < S; s += s_stride) {
    float* a = pa + s;
    const float* b = pb + s;
    float Ac = 1.f, bc = 0.f;   // the lane's chunk as one map
    for (int n = n0; n < n1; ++n) { const float An = a[n * S]; bc = fmaf(An, bc, b[n * S]); Ac *= An; }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {   // inclusive scan of the maps over the lanes (later map o earlier map)
      const float Ap = __shfl_up(Ac, off, 64), bp = __shfl_up(bc, off, 64);
      if (lane >= off) { bc = fmaf(Ac, bp, bc); Ac *= Ap; }
    }
    float Ae = __shfl_up(Ac, 1, 64), be = __shfl_up(bc, 1, 64);
    if (lane == 0) { Ae = 1.f; be = 0.f; }
    float x = fmaf(Ae, x0[s], be);
    for (int n = n0; n < n1; ++n) { x = fmaf(a[n * S], x, b[n * S]); a[n * S] = x; }
  }
}

// ---- label heads ------------------------------------------------------------------------------------------------
// logits lg[0 .. u_dim) of label head a on the latents zz (the head's own dims), half-wave = head, lane j32 = hidden unit.  Every lane of the
// wave takes part in every sum (columns beyond u_dim add zeros): call from wave-uniform control flow.
// (The per-kind log-probability stays with the callers: eval_stats forms its hit test inside the same loops, from the same exponentials.)
__device__ __forceinline__ void fwd_label_logits(const LabelHeadK& k, const float* __restrict__ par, int a, const float* zz, int j32, float (&lg)[8]) {
  const int zd = k.aux[a].z_dim, ud = k.aux[a].u_dim, U = k.U;
  const bool unit_on = j32 < U;
  const int jj = min(j32, U - 1);
  float pre = par[k.aux_b1[a] + jj];
  for (int l = 0; l < zd; ++l) pre = fmaf(par[k.aux_w1[a] + jj * zd + l], zz[l], pre);
  const float hv = unit_on ? softplusf(pre) : 0.f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const float w = (q < ud) ? par[k.aux_w2[a] + min(q, ud - 1) * U + jj] : 0.f;
    lg[q] = half_wave_sum(w * hv) + par[k.aux_b2[a] + min(q, ud - 1)];
  }
}

// ---- staged weights (recon, bounds, intervene) ----------------------------------------------------------------------
// offsets (in floats, multiples of 4) of the shared pieces of the dynamic LDS region; each kernel's own pieces follow them
struct FwdLds { int a, b, row, w1, b1, w2, hw, bgd, z, u, h0, x0; };
struct LdsCarve {
  int n = 0;
  int take(int c) { const int at = n; n += (c + 3) & ~3; return at; }
};
// generic: the run-time-S instantiation (rows sized for SLODE_MAX_S)
inline FwdLds fwd_lds(LdsCarve& cv, const slode_shape& s, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3, RW = FWD_ROW(generic ? SLODE_MAX_S : s.S);
  FwdLds o{};
  o.a = cv.take((s.T - 1) * s.S); o.b = cv.take((s.T - 1) * s.S); o.row = cv.take(s.H * RW);
  o.w1 = cv.take(s.L * 2 * s.H); o.b1 = cv.take(2 * s.H); o.w2 = cv.take(s.H * s.S + s.S); o.hw = cv.take(Q * s.C * s.S); o.bgd = cv.take(2 * s.S);
  o.z = cv.take(s.L); o.u = cv.take(s.n_u > 0 ? s.n_u : 1); o.h0 = cv.take(s.H); o.x0 = cv.take(s.S);
  return o;
}

struct FwdSm {
  float* A;     // A[T-1][S], overwritten by x[n+1][.] in the scan
  float* B;     // b[T-1][S]
  float* row;   // [H][RW]: w_t | u_j (per solve) | W_g[0..S)[j] | W_d[0..S)[j]
  float* w1;    // [L][2H]: z-columns of the hidden layer (r < H) and the init net's first layer (r >= H), transposed
  float* b1;    // [2H]
  float* w2;    // [H][S] init net's output layer, transposed | [S] its bias
  float* hw;    // [Q*C][S] head weights
  float* bgd;   // [2S] growth | degradation bias
  float *z, *u, *h0, *x0;
};
__device__ __forceinline__ FwdSm fwd_sm(float* base, const FwdLds& o) {
  return FwdSm{base + o.a, base + o.b, base + o.row, base + o.w1, base + o.b1, base + o.w2, base + o.hw, base + o.bgd,
               base + o.z, base + o.u, base + o.h0, base + o.x0};
}

// once per workgroup: the weights every solve reuses, into the LDS (a barrier must follow before they are read)
template <int SM>
__device__ __forceinline__ void fwd_stage_weights(const FwdK& k, const FwdSm& m, int S, int tid) {
  constexpr int RW = FWD_ROW(SM);
  const float* __restrict__ par = k.params;
  const int L = k.L, H = k.H, C = k.C, QC = k.Q * k.C;
  for (int i = tid; i < H * RW; i += FWD_NT) {
    const int j = i / RW, c = i - j * RW;
    float v = 0.f;
    if (c == 0) v = par[k.dyn_wh + j * (1 + L)];
    else if (c >= 2 && c < 2 + S) v = par[k.dyn_wg + (c - 2) * H + j];
    else if (c >= 2 + SM && c < 2 + SM + S) v = par[k.dyn_wd + (c - 2 - SM) * H + j];
    m.row[i] = v;
  }
  for (int i = tid; i < L * 2 * H; i += FWD_NT) {
    const int l = i / (2 * H), r = i - l * 2 * H;
    m.w1[i] = r < H ? par[k.dyn_wh + r * (1 + L) + 1 + l] : par[k.init_w1 + (r - H) * L + l];
  }
  for (int i = tid; i < 2 * H; i += FWD_NT) m.b1[i] = i < H ? par[k.dyn_bh + i] : par[k.init_b1 + i - H];
  for (int i = tid; i < H * S + S; i += FWD_NT) {
    const int j = i / S, s = i - j * S;
    m.w2[i] = i < H * S ? par[k.init_w2 + s * H + j] : par[k.init_b2 + i - H * S];
  }
  for (int i = tid; i < QC * S; i += FWD_NT) {
    const int qc = i / S, q = qc / C;
    m.hw[i] = par[k.head[q] + (qc - q * C) * S + (i - qc * S)];
  }
  for (int i = tid; i < 2 * S; i += FWD_NT) m.bgd[i] = i < S ? par[k.dyn_bg + i] : par[k.dyn_bd + i - S];
}

// per solve, from z in m.z: u = W_z z + b_h into the units' rows and the init net's hidden layer; then x0.  Contains the barrier between
// the hidden layer and x0: call from workgroup-uniform control flow only.  (x0 and the rows are visible after the caller's next barrier.)
template <int SM>
__device__ __forceinline__ void fwd_init_state(const FwdSm& m, int H, int L, int S, int tid) {
  constexpr int RW = FWD_ROW(SM);
  if (tid < 2 * H) {
    float v = m.b1[tid];
    for (int l = 0; l < L; ++l) v = fmaf(m.w1[l * 2 * H + tid], m.z[l], v);
    if (tid < H) m.row[tid * RW + 1] = v;
    else m.h0[tid - H] = fmaxf(v, 0.f);
  }
  __syncthreads();
  if (tid < S) {
    float o = m.w2[H * S + tid];
    for (int j = 0; j < H; ++j) o = fmaf(m.w2[j * S + tid], m.h0[j], o);
    m.x0[tid] = sigmoidf_fast(o);
  }
}

// a(t, z), d(t, z) of one stage time from the LDS rows [w_t | u_j | W_g[.][j] | W_d[.][j]] (every lane reads the same address: broadcast)
// (rows are RW = 2 + 2 SM floats rounded up to a multiple of four, 16-byte aligned: read as 16-byte LDS loads)
template <int SM>
__device__ __forceinline__ void fwd_ad(const float* __restrict__ s_row, const float* __restrict__ s_bgd, int H, float t, int S,
                                       float (&a)[SM], float (&d)[SM]) {
  typedef float f4_t __attribute__((ext_vector_type(4)));
  constexpr int RW = FWD_ROW(SM);
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

// the staged form of the step table: the steps [n_lo, n_hi) on all four waves
template <int SM>
__device__ __forceinline__ void fwd_step_table_staged(const FwdK& k, const FwdSm& m, int S, int n_lo, int n_hi, int tid) {
  const float* s_row = m.row; const float* s_bgd = m.bgd;
  const int H = k.H;
  fwd_step_table<SM>(k, S, n_lo, n_hi, tid, FWD_NT, m.A, m.B, [&](float t, float (&a)[SM], float (&d)[SM]) { fwd_ad<SM>(s_row, s_bgd, H, t, S, a, d); });
}

// ---- the draw loop ------------------------------------------------------------------------------------------
// the LDS pieces loc | scale of one source of draws, carved where the kernel's own order of pieces has them
struct LocScLds { int loc, sc; };
inline LocScLds fwd_lds_loc_sc(LdsCarve& cv, const slode_shape& s) {
  LocScLds o{};
  o.loc = cv.take(s.L); o.sc = cv.take(s.L);
  return o;
}

// M1, once per trajectory b: the labels into m.u (only the conditional prior nets read them); loc / scale of the posterior (from the
// encoder launch) or of the conditional prior nets -- N(0, 1) on the dims outside every prior group -- into s_loc / s_sc, each read back
// by its own thread alone.  Contains two barriers (before: the staged weights' writes and the previous trajectory's readers of m.u / s_loc /
// s_sc; between the labels and the prior nets): call from workgroup-uniform control flow only.
__device__ __forceinline__ void fwd_draw_source(const DrawsK& k, const FwdSm& m, float* s_loc, float* s_sc, int b, int tid) {
  const int L = k.f.L;
  __syncthreads();
  if (!k.is_post && k.pr.n_groups > 0 && tid < k.pr.nu) m.u[tid] = slode_label_at(k.lab, k.u, k.pr.nu, b, tid);
  __syncthreads();
  if (tid < L) {
    const int l = tid;
    float loc, sc;
    if (k.is_post) {
      loc = k.loc[(long long)b * L + l]; sc = k.scale[(long long)b * L + l];
    } else {
      float pl, pls;
      fwd_prior_at(k.pr, k.f.params, m.u, l, pl, pls);
      loc = pl; sc = expf(pls);
    }
    s_loc[l] = loc; s_sc[l] = sc;
  }
}

// M2: z of draw kk of trajectory b into m.z = loc + scale * eps, eps row kk * B + b of ONE drawing call or of the explicit [ns, B, L] tensor
// (the caller's barrier follows)
__device__ __forceinline__ void fwd_draw_z(const DrawsK& k, const FwdSm& m, const float* s_loc, const float* s_sc, int kk, int b, int tid) {
  if (tid < k.f.L) m.z[tid] = fmaf(s_sc[tid], slode_eps_at(k.rng, k.eps, (long long)kk * k.f.B + b, k.f.L, tid), s_loc[tid]);
}

// M3 - M5, one solve of the steps [n_lo, n_hi) from the z in m.z (visible: the caller's barrier) on all four waves: fwd_init_state (the
// units' rows of this z; x0), the step table, the scan from x_init -- m.x0 for a solve from the grid's start, a carried state otherwise.
// Afterwards the state after step n_lo + i is m.A[i][.].  Contains fwd_init_state's barrier, one after the table and one after the scan:
// call from workgroup-uniform control flow only.
template <int SM>
__device__ __forceinline__ void fwd_solve(const FwdK& k, const FwdSm& m, int S, const float* x_init, int n_lo, int n_hi, int tid) {
  fwd_init_state<SM>(m, k.H, k.L, S, tid);
  fwd_step_table_staged<SM>(k, m, S, n_lo, n_hi, tid);
  __syncthreads();
  fwd_scan(m.A, m.B, x_init, S, n_hi - n_lo, tid & 63, tid >> 6, FWD_NT / 64);
  __syncthreads();
}

// M6: the state of point j of the solved range (j = 0: x0; else the scanned m.A[j - 1]) ...
template <int SM>
__device__ __forceinline__ void fwd_state_at(const FwdSm& m, int S, int j, float (&x)[SM]) {
#pragma unroll
  for (int s = 0; s < SM; ++s) x[s] = s < S ? (j == 0 ? m.x0[s] : m.A[(j - 1) * S + s]) : 0.f;
}
// ... and the value of head row qc = q * C + c on it
template <int SM>
__device__ __forceinline__ float fwd_head_value(const FwdSm& m, int S, int qc, const float (&x)[SM]) {
  float v = 0.f;
#pragma unroll
  for (int s = 0; s < SM; ++s) if (s < S) v = fmaf(m.hw[qc * S + s], x[s], v);
  return v;
}

// The running moments of one value over the draws, shifted by the first draw's value: m[0] = v0, m[P] = s1 = sum (v - v0), m[2 P] = s2 =
// sum (v - v0)^2 (P: the slot stride of the kernel's table) -- no sum of v^2, whose fp32 rounding would exceed the variance of a
// prior-pass curve.  One owner thread per value, draws in order.  Returns v - v0 (0 on the first draw).
__device__ __forceinline__ float fwd_moment_add(float* m, int P, bool first, float v) {
  if (first) { m[0] = v; m[P] = 0.f; m[2 * P] = 0.f; return 0.f; }
  const float dv = v - m[0];
  m[P] += dv; m[2 * P] = fmaf(dv, dv, m[2 * P]);
  return dv;
}
// M7: mean = v0 + s1 / ns and sd = sqrt(max(0, s2 - s1^2 / ns) / ns) to element o of the outputs that were asked for (inv = 1 / ns)
__device__ __forceinline__ void fwd_moment_store(const float* m, int P, float inv, float* mean, float* sd, long long o) {
  const float s1 = m[P], s2 = m[2 * P];
  if (mean) mean[o] = fmaf(s1, inv, m[0]);
  if (sd) sd[o] = sqrtf(fmaxf(s2 - s1 * s1 * inv, 0.f) * inv);
}
// M7 with the operation order pinned -- mean = fma(s1, inv, v0); sd = sqrt(max(s2 - (s1 s1) inv, 0) inv), every product and the difference
// rounded on its own (no contraction into an fma) -- so that the result is bitwise the numpy restatement of the accumulation
// (tests/recon_moments_util.py: shifted_moments_f32), whatever the compiler would fuse.  The mean is always stored.
__device__ __forceinline__ void fwd_moment_store_pinned(const float* m, int P, float inv, float* mean, float* sd, long long o) {
#pragma clang fp contract(off)
  const float s1 = m[P], s2 = m[2 * P];
  mean[o] = fmaf(s1, inv, m[0]);
  if (sd) {
    const float sq = s1 * s1, sub = sq * inv;
    sd[o] = sqrtf(fmaxf(s2 - sub, 0.f) * inv);
  }
}

// one value into a sorted LDS buffer of depth m (slot stride P) that holds min(kk, m) values: BOTTOM: the smallest so far, ascending; else the
// largest so far, descending (recon_quantiles_kernel's M6, pointwise_loo_kernel's tail buffer)
template <bool BOTTOM>
__device__ __forceinline__ void fwd_sorted_insert(float* buf, int P, int m, int kk, float v) {
  int j = kk;
  if (kk >= m) {
    const float last = buf[(m - 1) * P];
    if (!(BOTTOM ? v < last : v > last)) return;
    j = m - 1;
  }
  while (j > 0) {
    const float prev = buf[(j - 1) * P];
    if (!(BOTTOM ? prev > v : prev < v)) break;
    buf[j * P] = prev;
    --j;
  }
  buf[j * P] = v;
}

// ---- launch ---------------------------------------------------------------------------------------------------------
// the run-time-S instantiation serves every state dim without a compiled one, and every shape under SLODE_ODE_GENERIC
inline bool fwd_generic(const slode_shape& s, int force_generic) { return force_generic || !(s.S == 5 || s.S == 8); }

// go(std::integral_constant<int, SC>) with SC the compile-time state dim of the shape: 5 (cvs / challenge), 8 (proc), 0 (run time)
template <class F>
inline void fwd_dispatch(const slode_shape& s, int force_generic, F&& go) {
  if (fwd_generic(s, force_generic)) go(std::integral_constant<int, 0>{});
  else if (s.S == 5) go(std::integral_constant<int, 5>{});
  else go(std::integral_constant<int, 8>{});
}
template <class K>
inline void fwd_launch(const char* name, void (*fn)(K), int grid, size_t lds, hipStream_t stream, const K& k) {
  if (lds > 48 * 1024) (void)hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  SLODE_LAUNCH(name, fn, dim3(grid), dim3(FWD_NT), lds, stream, k);
}

}  // namespace
