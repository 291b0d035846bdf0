// Pareto-smoothed importance-sampling leave-one-out (slode_pointwise_loo; Vehtari, Gelman & Gabry 2017, Vehtari et al. 2024): for every
// trajectory b and observation point i = (c, t), from the K posterior draws of slode_pointwise_density (posterior weights), with
//   l_k[i] = pointwise_kernel's per-draw log-density of the point (tb_point_loglik: the same routine, the same bits)
// the three planes
//   elpd_loo[i] = log sum_k w_k exp(l_k[i]),  w_k the normalised Pareto-smoothed importance ratios 1 / p(y_i | z_k)
//   khat[i]     = the shape of the generalised Pareto distribution fitted to the M largest ratios (+inf: no smoothing was possible)
//   lppd[i]     = log (1 / K) sum_k exp(l_k[i]), bit for bit plane 0 of slode_pointwise_density in posterior mode
// and eight sums per trajectory (SLODE_LOO_SLOTS).  Only the M + 1 smallest l_k of a point matter to the smoothing: they are kept sorted on
// chip (the insertion of recon_quantiles_kernel); no [B, C, T, K] tensor exists.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid), the frame of pointwise_kernel:
//   P0  staged weights, the likelihood scale table
//   P1  once per trajectory: labels, observations and mask [C][T]; the posterior of thread l
//   per sweep (a tile of `tile` time points; sweeps = ceil(T / tile)), per draw k = 0 .. K - 1, in that order:
//     P9  z (the same noise rows in every sweep), fwd_solve over the WHOLE grid (the curve bits do not depend on the tile), the
//         point fold: thread <-> time point t0 + tid, t0 + tid + 256, ... of the tile; for each of its C channels the thread alone owns the
//         point's LDS state [.][C][tile], t fastest: the lppd pair (max, sum) of lw + l_k exactly as pointwise_kernel keeps it, the bottom
//         buffer of depth M + 1, and a second pair for logsumexp(-l_k) over the draws OUTSIDE the buffer: a value that the buffer turns away
//         or pushes out has M + 1 smaller ones, so it is no tail draw whatever comes later.  (A sum over all K draws less the tail's own
//         terms cancels where one ratio dominates: at khat > 1 the smoothing shrinks the denominator to the size of that fp32 sum's rounding.)
//     P10 once per sweep: the owner runs loo_psis over its column in fp64 and stores the planes (and the kept tail)
//   P11 once per trajectory: the summary from the ROUNDED plane values, read back in the order of pointwise_kernel's P10 (thread <-> t = tid,
//       tid + 256, ...; (t, c)), whatever the tile; tb_wave_sum_d, the four waves as (0 + 1) + (2 + 3); two 16-byte stores
// loo_psis goes over the m <= 30 + floor(sqrt M) grid points of the Zhang & Stephens profile twice -- pass 1: the running maximum and sum of
// the L_j; pass 2: L_j again, the weights, b* -- and holds no per-thread array: no scratch.
// Every sum runs in a fixed order that depends on (K, C, T, L) alone and every per-point value has one owner: all outputs are bitwise equal
// between runs, grids, tiles and noise sources.  No atomics.
#include <float.h>
#include "traj_terms.h"

namespace {

constexpr int LOO_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then this kernel's own
struct LooLds { FwdLds f; ScoredLds s; int sum, pm, ps, nm, ns, buf, total; };

struct LooK {
  FwdK f;
  PriorK pr;
  ScoredK d;
  float lw_u;   // -log K (K = 1: +0), the log-weight of pointwise_kernel's posterior mode
  int tile, depth;   // depth = M + 1
  float *point, *summary, *tail;
  LooLds o;
};

// P9's fold of one draw into the state of the tile's points
template <int SM>
__device__ __forceinline__ void loo_fold_points(const FwdSm& sm, int S, int T, int C, int Q, int gauss, const float (&tau)[3], const float* s_obs,
                                                const float* s_inv, const float* s_lg, float* s_pm, float* s_ps, float* s_nm, float* s_ns,
                                                float* s_buf, int t0, int tn, int tile, int depth, int kk, float lw, int tid) {
  const int P = C * tile;
  for (int tl = tid; tl < tn; tl += LOO_NT) {
    const int t = t0 + tl;
    float x[SM];
    fwd_state_at<SM>(sm, S, t, x);
    for (int c = 0; c < C; ++c) {
      const int i = c * T + t, j = c * tile + tl;
      const float obv = s_obs[i], inv = s_inv[i], lg = s_lg[i];
      const float l = tb_point_loglik<SM>(sm, S, C, Q, c, gauss, tau, obv, inv, lg, x);
      const float a = lw + l;
      if (kk == 0) { s_pm[j] = a; s_ps[j] = 1.f; s_nm[j] = -INFINITY; s_ns[j] = 0.f; }
      else {
        const float m = s_pm[j];
        if (a > m) { s_ps[j] = fmaf(s_ps[j], expf(m - a), 1.f); s_pm[j] = a; }
        else s_ps[j] += expf(a - m);
      }
      if (kk >= depth) {   // the buffer is full: the draw that stays outside it -- this one, or the one it pushes out
        const float last = s_buf[(depth - 1) * P + j], v = -(l < last ? last : l), n = s_nm[j];
        if (v > n) { s_ns[j] = fmaf(s_ns[j], expf(n - v), 1.f); s_nm[j] = v; }   // (the first: n = -inf, exp = 0, the sum 1)
        else s_ns[j] += expf(v - n);
      }
      fwd_sorted_insert<true>(s_buf + j, P, depth, kk, l);
    }
  }
}

// mean_i log1p(-b x_i) over the tail x_i = exp(l_(0) - l_(n-1-i)) - ec, i = 0 .. n - 1 (ascending), from the sorted column
__device__ __forceinline__ double loo_profile_k(const float* col, int P, int n, double l0, double ec, double b) {
  double acc = 0.0;
  for (int i = 0; i < n; ++i) acc += log1p(-b * (exp(l0 - (double)col[(n - 1 - i) * P]) - ec));
  return acc / (double)n;
}

// Steps 2 - 6 of one point in fp64, from its sorted column l_(0) <= ... <= l_(M) (slot stride P) and the pair (nm, ns) of the K - M - 1
// draws outside it: sum exp(-l_k) = ns exp(nm) (none: ns = 0).  Left to the inliner (inlined, P10 costs the kernel ~20 VGPRs; as a call it needed a scratch frame for the callee-saved registers).
__device__ float2 loo_psis(const float* col, int P, int M, int K, float nm, float ns) {
  const double LOG_MIN = -708.39641853226408;   // log DBL_MIN
  const double l0 = (double)col[0];
  const double aM = l0 - (double)col[M * P];
  const double cut = fmax(aM, LOG_MIN), ec = exp(cut);
  int n = 0;   // the tail: ranks 0 .. n - 1 (a is non-increasing in the rank; a tie with the cutoff drops out)
  while (n < M && l0 - (double)col[n * P] > cut) ++n;
  double khat = INFINITY, sigma = 0.0;
  bool smooth = false;
  if (n >= 5) {
    const int m = 30 + (int)floor(sqrt((double)n));
    const double xq = exp(l0 - (double)col[(n - (int)((double)n / 4.0 + 0.5)) * P]) - ec;   // x_[floor(n / 4 + 0.5) - 1]
    const double xn = 1.0 - ec;                                                               // x_[n - 1]: rank 0
    const double dn = (double)n, dm = (double)m, ib = 1.0 / (3.0 * xq), ix = 1.0 / xn;
    double lmax = -INFINITY, lsum = 0.0;
    for (int j = 1; j <= m; ++j) {   // pass 1: the maximum and the shifted sum of the profile log-likelihoods
      const double b = (1.0 - sqrt(dm / ((double)j - 0.5))) * ib + ix;
      const double kj = loo_profile_k(col, P, n, l0, ec, b);
      const double L = dn * (log(-b / kj) - kj - 1.0);
      if (L > lmax) { lsum = lsum * exp(lmax - L) + 1.0; lmax = L; }
      else lsum += exp(L - lmax);
    }
    double wsum = 0.0, bsum = 0.0;
    for (int j = 1; j <= m; ++j) {   // pass 2: the weights (those below 10 ulp dropped) and b*
      const double b = (1.0 - sqrt(dm / ((double)j - 0.5))) * ib + ix;
      const double kj = loo_profile_k(col, P, n, l0, ec, b);
      const double L = dn * (log(-b / kj) - kj - 1.0);
      const double w = exp(L - lmax) / lsum;
      if (w >= 10.0 * DBL_EPSILON) { wsum += w; bsum = fma(w, b, bsum); }
    }
    const double bs = bsum / wsum;
    const double ks = loo_profile_k(col, P, n, l0, ec, bs);
    sigma = -ks / bs;
    const double kh = (dn * ks + 5.0) / (dn + 10.0);
    if (isfinite(kh) && isfinite(sigma)) { khat = kh; smooth = true; }
  }
  // step 6, everything relative to exp(l_(0)): the numerator shifted by h = -cut >= every exponent below
  const double h = -cut;
  double num = (double)(K - n) * exp(-h), den_tail = 0.0;
  for (int i = 1; i <= n; ++i) {   // x ascending: rank n - i
    const double a = l0 - (double)col[(n - i) * P];
    double s = a;
    if (smooth) {
      const double p = ((double)i - 0.5) / (double)n;
      s = fmin(log(sigma * expm1(-khat * log1p(-p)) / khat + ec), 0.0);
    }
    den_tail += exp(s);
    num += exp(s - a - h);
  }
  // the draws outside the tail: the kept ranks n .. M (fp64) and the draws outside the buffer (their fp32 pair, shifted to l_(0))
  double rest = ns > 0.f ? (double)ns * exp((double)nm + l0) : 0.0;
  for (int j = M; j >= n; --j) rest += exp(l0 - (double)col[j * P]);
  return make_float2((float)(l0 + h + log(num) - log(rest + den_tail)), (float)khat);   // (elpd_loo, khat)
}

// P10 of one sweep: the planes (and the kept tail) of the thread's points of the tile
__device__ __forceinline__ void loo_store_points(const float* s_pm, const float* s_ps, const float* s_nm, const float* s_ns, const float* s_buf, int T, int C, int t0, int tn,
                                                 int tile, int depth, int K, long long B, long long b, float* point, float* tail, int tid) {
  const int P = C * tile;
  const long long plane = B * C * T;
  for (int tl = tid; tl < tn; tl += LOO_NT)
    for (int c = 0; c < C; ++c) {
      const int j = c * tile + tl;
      const long long o = (b * C + c) * T + t0 + tl;
      const float2 ek = loo_psis(s_buf + j, P, depth - 1, K, s_nm[j], s_ns[j]);
      point[o] = ek.x; point[plane + o] = ek.y; point[2 * plane + o] = s_pm[j] + logf(s_ps[j]);
      if (tail)
        for (int r = 0; r < depth; ++r) tail[r * plane + o] = s_buf[r * P + j];
    }
}

// P11: the summary of trajectory b from the stored planes (visible: the caller's fence and barrier).  Not inlined, as pw_finish.
__device__ __noinline__ void loo_summary(const float* point, const float* s_w, double* s_sum, int T, int C, long long B, long long b, float* summary) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long plane = B * C * T;
  double acc[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) acc[j] = 0.0;
  float kmax = -INFINITY;
  for (int t = tid; t < T; t += LOO_NT)
    for (int c = 0; c < C; ++c) {
      const long long o = (b * C + c) * T + t;
      const float elpd = point[o], khat = point[plane + o], lppd = point[2 * plane + o];
      if (s_w[c * T + t] > 0.f) {
        acc[0] += (double)elpd; acc[1] += (double)lppd; acc[2] += 1.0;
        if (khat > 0.7f) acc[3] += 1.0;
        kmax = fmaxf(kmax, khat);
      } else { acc[4] += (double)elpd; acc[5] += (double)lppd; acc[6] += 1.0; }
    }
#pragma unroll
  for (int j = 0; j < 7; ++j) acc[j] = tb_wave_sum_d(acc[j]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) kmax = fmaxf(kmax, __shfl_xor(kmax, off, 64));
  if (lane == 0) {
#pragma unroll
    for (int j = 0; j < 7; ++j) s_sum[wave * 8 + j] = acc[j];
    s_sum[wave * 8 + 7] = (double)kmax;
  }
  __syncthreads();
  if (tid == 0) {
    typedef float f4_t __attribute__((ext_vector_type(4)));
    float v[7];
#pragma unroll
    for (int j = 0; j < 7; ++j) v[j] = (float)((s_sum[j] + s_sum[8 + j]) + (s_sum[16 + j] + s_sum[24 + j]));
    const float km = (float)fmax(fmax(s_sum[7], s_sum[15]), fmax(s_sum[23], s_sum[31]));
    f4_t lo, hi;
    lo.x = v[0]; lo.y = v[1]; lo.z = v[2]; lo.w = v[3]; hi.x = km; hi.y = v[4]; hi.z = v[5]; hi.w = v[6];
    f4_t* row = reinterpret_cast<f4_t*>(summary + b * SLODE_LOO_SLOTS);
    row[0] = lo; row[1] = hi;   // the row's eight slots: two 16-byte stores
  }
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(LOO_NT) pointwise_loo_kernel(const LooK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_loo[];
  const FwdK& f = k.f;
  const int tid = threadIdx.x, T = f.T, L = f.L, S = SC ? SC : f.S, C = f.C, Q = f.Q, nd = k.d.nd, tile = k.tile, depth = k.depth;
  const FwdSm sm = fwd_sm(s_loo, k.o.f);
  const ScoredSm ss = scored_sm(s_loo, k.o.s);
  float* s_pm = s_loo + k.o.pm;     // [C][tile] running maximum of lw + l_k
  float* s_ps = s_loo + k.o.ps;     // [C][tile] sum of exp(lw + l_k - max)
  float* s_nm = s_loo + k.o.nm;     // [C][tile] running maximum of -l_k over the draws outside the buffer
  float* s_ns = s_loo + k.o.ns;     // [C][tile] sum of exp(-l_k - max)
  float* s_buf = s_loo + k.o.buf;   // [depth][C][tile] the depth smallest l_k so far, ascending
  double* s_sum = reinterpret_cast<double*>(s_loo + k.o.sum);   // [4][8] per-wave partials of the summary

  // ---- P0 ----
  fwd_stage_weights<SM>(f, sm, S, tid);
  tb_stage_scales(k.d, ss, C * T, tid);

  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    // ---- P1 ----
    __syncthreads();   // (P0's writes; the previous trajectory's readers of every table are done)
    if (tid < k.pr.nu) sm.u[tid] = slode_label_at(k.d.lab, k.d.u, k.pr.nu, b, tid);
    tb_stage_obs<true>(k.d, ss, b, T, C, tid);
    __syncthreads();
    TbDim q;
    if (tid < L) tb_dim_load(q, k.d, k.pr, f.params, sm.u, b, L, tid, false);
    for (int t0 = 0; t0 < T; t0 += tile) {
      const int tn = min(tile, T - t0);
      // ---- P9 ----
      for (int kk = 0; kk < nd; ++kk) {
        if (tid < L) sm.z[tid] = fmaf(q.sc, slode_eps_at(k.d.rng, k.d.eps, b, L, tid, kk, f.B), q.loc);
        __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 are done)
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);
        loo_fold_points<SM>(sm, S, T, C, Q, k.d.gauss, k.d.tau, ss.obs, ss.inv, ss.lg, s_pm, s_ps, s_nm, s_ns, s_buf, t0, tn, tile, depth, kk, k.lw_u, tid);
      }
      // ---- P10: the owners' own values: no barrier needed ----
      loo_store_points(s_pm, s_ps, s_nm, s_ns, s_buf, T, C, t0, tn, tile, depth, nd, f.B, b, k.point, k.tail, tid);
    }
    // ---- P11 ----
    __threadfence_block();
    __syncthreads();   // (the planes of this trajectory, stored by the tiles' owners, are visible to the workgroup)
    loo_summary(k.point, ss.w, s_sum, T, C, f.B, b, k.summary);
  }
}

LooLds loo_lds(const slode_shape& s, int depth, int tile, bool generic) {
  const int CP = s.C * tile;
  LdsCarve cv;
  LooLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.s = scored_lds(cv, s, true, 0, 0);
  o.sum = cv.take(64);
  o.pm = cv.take(CP); o.ps = cv.take(CP); o.nm = cv.take(CP); o.ns = cv.take(CP);
  o.buf = cv.take(depth * CP);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_pointwise_loo_lds_bytes(const slode_shape& s, int depth, int tile, int force_generic) {
  if (depth < 1 || tile < 1 || (long long)depth * s.C * tile > (1 << 26)) return (size_t)1 << 30;   // (far beyond any budget; keeps the carve's int arithmetic in range)
  return (size_t)loo_lds(s, depth, tile, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_pointwise_loo(const PointwiseLooLaunch& a, hipStream_t stream) {
  const ScoredLaunch& d = a.d;
  const slode_shape& s = d.s;
  if (d.num_draws < 1 || d.grid < 1 || !a.point || !a.summary || a.tile < 1 || a.tile > s.T || a.depth < 1 || a.depth > d.num_draws)
    return hipErrorInvalidValue;
  const size_t lds = slode_pointwise_loo_lds_bytes(s, a.depth, a.tile, d.force_generic);
  if (lds > SLODE_LOO_LDS_MAX) return hipErrorInvalidValue;
  LooK k{};
  fwd_fill(k.f, s, d.lay, d.params, d.times, d.stage_t); fwd_fill(k.pr, s, d.lay); fwd_fill(k.d, d);
  k.lw_u = (float)(0.0 - log((double)d.num_draws));
  k.tile = a.tile; k.depth = a.depth;
  k.point = a.point; k.summary = a.summary; k.tail = a.tail_out;
  k.o = loo_lds(s, a.depth, a.tile, fwd_generic(s, d.force_generic));
  fwd_dispatch(s, d.force_generic, [&](auto sc) { fwd_launch("pointwise_loo", pointwise_loo_kernel<decltype(sc)::value>, d.grid, lds, stream, k); });
  return hipGetLastError();
}
