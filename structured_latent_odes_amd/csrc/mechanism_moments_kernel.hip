// Mechanism curves (slode_mechanism_moments): per trajectory, the mean and the population standard deviation over num_samples latent draws of
// what the dynamics dx/dt = a(t, z) - d(t, z) x say at every grid point -- the state x, the production a, the degradation d, the set point
// a / d and the net rate a - d x -- without writing anything sized num_samples x B x T x S.
// One workgroup of four waves handles one trajectory at a time (persistent loop beyond the grid) and walks its draws k = 0 .. ns - 1 in
// that order: the draw loop of slode_forward.h with one addition, the capture of each step's first stage:
//   M0  once per workgroup: fwd_stage_weights
//   M1  once per trajectory: fwd_draw_source
//   per draw: M2 fwd_draw_z; M3 fwd_init_state; M4 the step table, thread <-> step, around fwd_step_coeffs with a wrapped evaluator: the first
//       evaluation of step n is the one at stage_t[n R], bitwise times[n], and is also written to the capture table [T][2 S]; the thread
//       whose turn point T - 1 is takes one fwd_ad at stage_t[R (T - 1)], bitwise times[T - 1], and no step; M5 fwd_scan
//   M6  thread <-> time point: x_t from the scan, a, d from the capture table (the thread's own writes), the selected slots and their running
//       moments (fwd_moment_add), table [n_sel][S][3][T]
//   M7  once per trajectory: fwd_moment_store_pinned, written with T contiguous
// The routines and the operation order of the solve are those of fwd_solve: the states are bitwise those of recon_moments on the same noise.
// The moments of (slot, s, t) belong to ONE thread for the whole trajectory and take the draws in the fixed order k = 0 .. ns - 1: the
// result is a function of (parameters, inputs, noise) alone -- independent of the grid and of which slots are asked for, bitwise
// reproducible, no atomics.
#include "slode_forward.h"

namespace {

constexpr int MM_NT = FWD_NT;

// offsets (in floats, multiples of 4) of the pieces of the dynamic LDS region: the shared ones, then the moments, loc | scale and the capture
struct MmLds { FwdLds f; int acc; LocScLds ls; int cap; int total; };

struct MmK {
  DrawsK d;
  float *mean, *sd;
  unsigned int slots;
  MmLds o;
};

// floats of one slot's moment triples [S][3][T], rounded up to a multiple of four: a further slot costs exactly this much LDS
__host__ __device__ inline int mm_slot_floats(int S, int T) { return (3 * S * T + 3) & ~3; }

// SC: ode_state_dim at compile time (5: cvs / challenge, 8: proc), 0: any S <= SLODE_MAX_S at run time
template <int SC>
__global__ void __launch_bounds__(MM_NT) mechanism_moments_kernel(const MmK k) {
  constexpr int SM = SC ? SC : SLODE_MAX_S;
  extern __shared__ __attribute__((aligned(16))) float s_mm[];
  const FwdK& f = k.d.f;
  const int tid = threadIdx.x;
  const int T = f.T, S = SC ? SC : f.S, H = f.H, ns = k.d.ns;
  const unsigned int slots = k.slots;
  const FwdSm sm = fwd_sm(s_mm, k.o.f);
  float* s_acc = s_mm + k.o.acc;   // [n_sel][S][3: v0, s1, s2][T], a slot's 3 S T floats rounded up to a multiple of four
  const int slot_stride = mm_slot_floats(S, T);
  float* s_loc = s_mm + k.o.ls.loc;
  float* s_sc = s_mm + k.o.ls.sc;
  float* s_cap = s_mm + k.o.cap;   // [T][a[0..S) | d[0..S)] at the grid times
  const float* s_row = sm.row; const float* s_bgd = sm.bgd;

  fwd_stage_weights<SM>(f, sm, S, tid);   // M0
  for (int b = blockIdx.x; b < f.B; b += gridDim.x) {
    fwd_draw_source(k.d, sm, s_loc, s_sc, b, tid);   // M1
    for (int kk = 0; kk < ns; ++kk) {
      fwd_draw_z(k.d, sm, s_loc, s_sc, kk, b, tid);   // M2
      __syncthreads();   // (also: the previous draw's readers of s_A / s_x0 / s_row[.][1] are done)
      fwd_init_state<SM>(sm, H, f.L, S, tid);   // M3
      // ---- M4: the step table as fwd_step_table_staged builds it; the first stage of every step, and point T - 1, captured ----
      for (int i = tid; i < T; i += MM_NT) {
        float* cap = s_cap + i * 2 * S;
        bool first = true;
        auto ad = [&](float t, float (&a)[SM], float (&d)[SM]) {
          fwd_ad<SM>(s_row, s_bgd, H, t, S, a, d);
          if (first) {
            first = false;
#pragma unroll
            for (int s = 0; s < SM; ++s)
              if (s < S) { cap[s] = a[s]; cap[S + s] = d[s]; }
          }
        };
        if (i < T - 1) {
          float A[SM], bb[SM];
          fwd_step_coeffs<SM>(f.method, f.times[i + 1] - f.times[i], f.stage_t + (long long)i * f.R, ad, A, bb);
#pragma unroll
          for (int s = 0; s < SM; ++s)
            if (s < S) { sm.A[i * S + s] = A[s]; sm.B[i * S + s] = bb[s]; }
        } else {
          float a[SM], d[SM];
          ad(f.stage_t[(long long)f.R * (T - 1)], a, d);
        }
      }
      __syncthreads();
      fwd_scan(sm.A, sm.B, sm.x0, S, T - 1, tid & 63, tid >> 6, MM_NT / 64);   // M5
      __syncthreads();
      // ---- M6: the slots of the thread's time points, running moments ----
      for (int t = tid; t < T; t += MM_NT) {
        float x[SM];
        fwd_state_at<SM>(sm, S, t, x);
        const float* cap = s_cap + t * 2 * S;
#pragma unroll
        for (int s = 0; s < SM; ++s)
          if (s < S) {
            const float a = cap[s], d = cap[S + s];
            float v[SLODE_MECHANISM_SLOTS];
            v[0] = x[s]; v[1] = a; v[2] = d; v[3] = a / d; v[4] = fmaf(-d, x[s], a);
            int j = 0;
#pragma unroll
            for (int q = 0; q < SLODE_MECHANISM_SLOTS; ++q)
              if ((slots >> q) & 1u) { fwd_moment_add(s_acc + j * slot_stride + (s * 3) * T + t, T, kk == 0, v[q]); ++j; }
          }
      }
    }
    // ---- M7: the thread's own (slot, s, t): no barrier needed; lanes <-> consecutive t: coalesced stores ----
    const float inv = 1.0f / (float)ns;
    const int rows = __popc(slots) * S;
    for (int t = tid; t < T; t += MM_NT)
      for (int r = 0; r < rows; ++r) {
        const int j = r / S, s = r - j * S;
        fwd_moment_store_pinned(s_acc + j * slot_stride + (s * 3) * T + t, T, inv, k.mean, k.sd, (((long long)j * f.B + b) * S + s) * T + t);
      }
  }
}

MmLds mm_lds(const slode_shape& s, int n_sel, bool generic) {
  LdsCarve cv;
  MmLds o{};
  o.f = fwd_lds(cv, s, generic);
  o.acc = cv.take(n_sel * mm_slot_floats(s.S, s.T)); o.ls = fwd_lds_loc_sc(cv, s); o.cap = cv.take(2 * s.T * s.S);
  o.total = cv.n;
  return o;
}

}  // namespace

size_t slode_mechanism_lds_bytes(const slode_shape& s, int n_sel, int force_generic) {
  return (size_t)mm_lds(s, n_sel, fwd_generic(s, force_generic)).total * sizeof(float);
}

hipError_t slode_launch_mechanism_moments(const MechanismLaunch& a, hipStream_t stream) {
  const slode_shape& s = a.d.s;
  const int n_sel = __builtin_popcount(a.slots);
  MmK k{};
  fwd_fill(k.d, a.d);
  k.mean = a.mean; k.sd = a.sd; k.slots = a.slots; k.o = mm_lds(s, n_sel, fwd_generic(s, a.d.force_generic));
  const size_t lds = slode_mechanism_lds_bytes(s, n_sel, a.d.force_generic);
  if (lds > SLODE_MECHANISM_LDS_MAX || a.d.num_samples < 1 || a.d.grid < 1 || !a.mean || a.slots == 0 || (a.slots >> SLODE_MECHANISM_SLOTS)) return hipErrorInvalidValue;
  fwd_dispatch(s, a.d.force_generic, [&](auto sc) { fwd_launch("mechanism_moments", mechanism_moments_kernel<decltype(sc)::value>, a.d.grid, lds, stream, k); });
  return hipGetLastError();
}
