// Sample quantiles of the reconstruction (slode_recon_quantiles): per trajectory, head curve, channel and time point, up to
// SLODE_QUANTILE_MAX_LEVELS order statistics (numpy's "linear" quantiles) of the num_samples = K latent draws -- the credible band, the envelope,
// the median -- without a [B, C, T, K] tensor and without a sort of one.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid).  The frame is curve_summary_kernel's, the
// draw loop of slode_forward.h:
//   M0  once per workgroup: fwd_stage_weights; the level table (buffer slots of the two ranks of every level and the weight g) into the LDS
//   M1  once per trajectory: fwd_draw_source
//   per sweep (a tile of `tile` time points; sweeps = ceil(T / tile)), per draw k = 0 .. K - 1, in that order:
//     M2 fwd_draw_z, M3-M5 fwd_solve over the WHOLE grid [0, T - 1) -- every sweep redraws the same noise and solves the same steps, so the
//        curve bits are those slode_recon_moments accumulates whatever the tile (fwd_scan's chunking depends on the number of steps)
//     M6 thread <-> time point of the tile: the Q * C head values, each inserted into the thread's own two sorted LDS buffers --
//        bottom: the m_lo smallest values so far, ascending (slots 0 .. m_lo - 1); top: the m_hi largest so far, descending (slots m_lo ..
//        m_lo + m_hi - 1).  The first m draws fill a buffer (insertion sort); afterwards a value is compared with the buffer's last element
//        and shifted in only when it enters.
//   M7  once per sweep: the owner stores, per level, out = fma(g, v_hi - v_lo, v_lo) with the difference rounded on its own, T contiguous
// Buffers: [D = m_lo + m_hi][Q * C][tile] floats, t fastest: the lanes of a wave touch consecutive banks at every depth.  Every buffer column
// has ONE owner thread, which takes the draws in the fixed order: no barriers beyond the frame's, no atomics.  An order statistic is a
// selection among the draw values, so every output is a function of (parameters, inputs, noise, levels) alone: bitwise independent of the
// grid, of the tile and of where the noise comes from.  Non-finite curve values are not ordered: the result for such a column is unspecified.
#include "slode_forward.h"

namespace {

constexpr int RQ_NT = FWD_NT;
constexpr int RQ_LV = SLODE_QUANTILE_MAX_LEVELS;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, loc | scale, then the kernel's own
struct RqLds { FwdLds f; LocScLds ls; int lv, buf; int total; };

struct RqK {
  DrawsK d;
  float* out;
  int n_levels, tile, m_lo, m_hi;
  int slot_lo[RQ_LV], slot_hi[RQ_LV];   // buffer slots (bottom: the rank r; top: m_lo + K - 1 - r) of the two ranks of a level
  float g[RQ_LV];                       // the weight of the upper rank
  RqLds o;
};

// M7 of one level: the interpolation with its operation order pinned -- the difference rounded on its own, then one fma -- so that the result
// is bitwise the numpy restatement (tests/quantile_util.py: select), whatever the compiler would fuse
__device__ __forceinline__ float rq_lerp(float v_lo, float v_hi, float g) {
#pragma clang fp contract(off)
  const float dv = v_hi - v_lo;
  return fmaf(g, dv, v_lo);
}

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(RQ_NT) recon_quantiles_kernel(const RqK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_rq[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, C = f.C, QC = f.Q * C, ns = k.d.ns;
  const int tile = k.tile, m_lo = k.m_lo, m_hi = k.m_hi, n_levels = k.n_levels;
  const FwdSm sm = fwd_sm(s_rq, k.o.f);
  float* s_loc = s_rq + k.o.ls.loc;
  float* s_sc = s_rq + k.o.ls.sc;
  int* s_slot = reinterpret_cast<int*>(s_rq + k.o.lv);   // [2][RQ_LV]: lower | upper rank's slot
  float* s_g = s_rq + k.o.lv + 2 * RQ_LV;                // [RQ_LV]
  float* s_buf = s_rq + k.o.buf;                         // [D][Q*C][tile]
  const int P = QC * tile;                               // slot stride

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
#pragma unroll
  for (int i = 0; i < RQ_LV; ++i)   // (a compile-time index: the kernel arguments are never indexed by a run-time value)
    if (tid == i) { s_slot[i] = k.slot_lo[i]; s_slot[RQ_LV + i] = k.slot_hi[i]; s_g[i] = k.g[i]; }
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1 (its first barrier: the level table is visible)
    for (int t0 = 0; t0 < T; t0 += tile) {
      const int tn = min(tile, T - t0);
      for (int kk = 0; kk < ns; ++kk) {
        fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
        __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 are done)
        fwd_solve<SM>(f, sm, S, sm.x0, 0, T - 1, tid);   // M3 - M5
        // ---- M6: the thread's time points of the tile; its own buffers ----
        for (int tl = tid; tl < tn; tl += RQ_NT) {
          float x[SM];
          fwd_state_at<SM>(sm, S, t0 + tl, x);
          for (int qc = 0; qc < QC; ++qc) {
            const float v = fwd_head_value<SM>(sm, S, qc, x);
            float* col = s_buf + qc * tile + tl;
            fwd_sorted_insert<true>(col, P, m_lo, kk, v);
            if (m_hi > 0) fwd_sorted_insert<false>(col + m_lo * P, P, m_hi, kk, v);
          }
        }
      }
      // ---- M7: the owners' own values: no barrier needed ----
      for (int tl = tid; tl < tn; tl += RQ_NT)
        for (int qc = 0; qc < QC; ++qc) {
          const int q = qc / C, c = qc - q * C;
          const float* col = s_buf + qc * tile + tl;
          for (int lv = 0; lv < n_levels; ++lv) {
            const float v_lo = col[s_slot[lv] * P], v_hi = col[s_slot[RQ_LV + lv] * P];
            k.out[((((long long)lv * f.Q + q) * f.B + b) * C + c) * T + t0 + tl] = rq_lerp(v_lo, v_hi, s_g[lv]);
          }
        }
    }
  }
}

RqLds rq_lds(const slode_shape& s, int depth, int tile, bool generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  LdsCarve cv;
  RqLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.ls = fwd_lds_loc_sc(cv, s);
  o.lv = cv.take(3 * RQ_LV);
  o.buf = cv.take(depth * Q * s.C * tile);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_recon_quantiles_lds_bytes(const slode_shape& s, int depth, int tile, int force_generic) {
  const int Q = s.likelihood == SLODE_GAUSS ? 1 : 3;
  if ((long long)depth * Q * s.C * tile > (1 << 26)) return (size_t)1 << 30;   // (far beyond any budget; keeps the carve's int arithmetic in range)
  return (size_t)rq_lds(s, depth, tile, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_recon_quantiles(const ReconQuantilesLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  const int K = a.d.num_samples, D = a.depth_lo + a.depth_hi;
  if (K < 1 || a.d.grid < 1 || !a.out || a.n_levels < 1 || a.n_levels > RQ_LV || a.tile < 1 || a.tile > s.T || a.depth_lo < 1 || a.depth_hi < 0 ||
      D > K)
    return hipErrorInvalidValue;
  RqK k{};
  fwd_fill(k.d, a.d);
  k.out = a.out; k.n_levels = a.n_levels; k.tile = a.tile; k.m_lo = a.depth_lo; k.m_hi = a.depth_hi;
  for (int i = 0; i < RQ_LV; ++i) {
    const bool on = i < a.n_levels;
    k.slot_lo[i] = on ? a.slot_lo[i] : 0; k.slot_hi[i] = on ? a.slot_hi[i] : 0; k.g[i] = on ? a.g[i] : 0.f;
    if (k.slot_lo[i] < 0 || k.slot_lo[i] >= D || k.slot_hi[i] < 0 || k.slot_hi[i] >= D) return hipErrorInvalidValue;
  }
  k.o = rq_lds(s, D, a.tile, fwd_generic(s, a.d.force_generic));
  const size_t lds = slode_recon_quantiles_lds_bytes(s, D, a.tile, a.d.force_generic);
  if (lds > SLODE_RECON_QUANTILES_LDS_MAX) return hipErrorInvalidValue;
  fwd_dispatch(s, a.d.force_generic, [&](auto sc) { fwd_launch("recon_quantiles", recon_quantiles_kernel<decltype(sc)::value>, a.d.grid, lds, stream, k); });
  return hipGetLastError();
}
