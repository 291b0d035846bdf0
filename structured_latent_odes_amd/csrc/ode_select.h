// Which ode_elbo_kernel instantiation a launch takes, with what grid, block and dynamic LDS: decided here, once, by host arithmetic (no HIP
// call, no allocation), so that a host program can ask it (tests/ode_select).  ode_shapes: the named shapes, once;
// ode_select: launch -> OdeVariant or the refusal; ode_dispatch: OdeVariant -> F<its fourteen arguments>::run(...), the one list of the 47
// instantiations.  The LDS bytes come from the variant's own template arguments by the rule the kernel carves with (ode_variant_map).
#pragma once
#include "slode_common.h"
#include "fixed_step.h"
#include "ode_layout.h"
#include <stdio.h>

namespace {

// (ode_state_dim, time points, channels, latent dim, decoder heads, solver); ode_hidden_dim is 25 in all of them
struct OdeShape { int S, T, C, L, Q, method; };
enum { ODE_METRIC, ODE_C0, ODE_C2, ODE_C4, ODE_REF_DEFAULT, ODE_N_NAMED, ODE_GENERIC5 = ODE_N_NAMED, ODE_GENERIC8, ODE_N_SHAPES };
constexpr int ODE_H = 25;
constexpr OdeShape ode_shapes[ODE_N_SHAPES] = {
  {5, 200, 3, 8, 3, SLODE_RK4},        // metric: BASELINE configs [1] / [3]: cvs, latent 3+3+2, ALD
  {5, 100, 3, 4, 3, SLODE_RK4},        // c0: config [0]: cvs, latent 1+1+2
  {8, 100, 4, 50, 3, SLODE_RK4},       // c2: config [2] shapes: proc, fixed grid (the scorer of its dopri5 form: the same dims, euler)
  {5, 300, 4, 15, 1, SLODE_RK4},       // c4: config [4]: challenge, Gauss
  {5, 86, 3, 15, 3, SLODE_MIDPOINT},   // ref_default: training_cvs.py, config_cvs.py
  {5, 0, 0, 0, 0, -1}, {8, 0, 0, 0, 0, -1},   // the generic instantiations: everything but S read from the launch struct
};
inline int ode_heads(const slode_shape& s) { return s.likelihood == SLODE_GAUSS ? 1 : 3; }
inline bool ode_dims_are(const slode_shape& s, int i) {
  const OdeShape& n = ode_shapes[i];
  return s.H == ODE_H && s.S == n.S && s.T == n.T && s.C == n.C && s.L == n.L && ode_heads(s) == n.Q;
}
inline bool ode_shape_is(const slode_shape& s, int i) { return ode_dims_are(s, i) && s.method == ode_shapes[i].method; }
inline int ode_stage_times(const slode_shape& s) { return fixed_step_times(s.method) * (s.T - 1) + 1; }

// Would this launch take an instantiation that runs the encoder forward itself (ENCF)?  Metric shape, loop-free backward, product form.
// The step asks before it skips the encoder launch; ode_select asks again when the launch says enc_fuse.
inline bool ode_takes_encf(const slode_shape& s, bool bwd, int grid, bool ext, int force_loop, int force_generic, int alg, int pack) {
  return bwd && grid == s.B && ode_shape_is(s, ODE_METRIC) && s.Hc <= 52 && alg == 0 && !ext && !force_generic && !force_loop && !(pack && pack < 10);
}

struct OdeVariant {
  bool ok;      // false: refused (the reason is in err), nothing else is set
  int shape;    // row of ode_shapes
  int S, H; bool BWD; int T_, C_, L_, Q_, M_; bool RA, ONE; int ALG, PK; bool ENCF, SOFTB;   // ode_elbo_kernel's template arguments
  int grid, nthreads;   // workgroups (x; y = particles), threads of a workgroup
  size_t lds;           // dynamic LDS bytes
  int stn;              // floats of its stage buffer (LdsMap::stn): what P7 may stage there (stage_encw)
};
inline OdeVariant ode_variant(int shape, const OdeShape& n, int H, bool bwd, bool ra, bool one, int alg = 0, int pk = 1, bool encf = false, bool softb = false) {
  OdeVariant v{};
  v.shape = shape; v.S = n.S; v.H = H; v.BWD = bwd; v.T_ = n.T; v.C_ = n.C; v.L_ = n.L; v.Q_ = n.Q; v.M_ = n.method;
  v.RA = ra; v.ONE = one; v.ALG = alg; v.PK = pk; v.ENCF = encf; v.SOFTB = softb;
  return v;
}
// The LdsMap instantiation v carves for one trajectory of this launch: the head of ode_elbo_kernel, restated (nthreads = blockDim.x).
inline LdsMap ode_variant_map(const OdeVariant& v, const slode_shape& s, int npar, int n_aux_lds, int nthreads) {
  const int T = v.T_ ? v.T_ : s.T, C = v.C_ ? v.C_ : s.C, L = v.L_ ? v.L_ : s.L, Q = v.Q_ ? v.Q_ : ode_heads(s);
  const int n_stage_t = (v.M_ >= 0 && v.T_) ? fixed_step_times(v.M_) * (T - 1) + 1 : ode_stage_times(s);
  const int NT = v.T_ ? ode_threads_for(v.T_, v.Q_, v.C_, v.S) : nthreads;
  return lds_map(T, v.S, v.H, C, L, Q, n_stage_t, ode_cold_global(v.L_) ? ode_hot_floats(v.S, v.H) : npar, NT, n_aux_lds, v.ONE, v.ALG == 3);
}
constexpr size_t ODE_LDS_MAX = 160 * 1024;

// npar: floats of the parameter segment [ode_begin, cstd); n_aux_lds: label heads that get LDS rows (OdeK::npar, OdeK::n_aux_lds)
inline OdeVariant ode_select(const OdeLaunch& a, int npar, int n_aux_lds, char* err, size_t errlen) {
  const slode_shape& s = a.s;
  const slode_layout& lay = a.lay;
  const int nthreads = ode_threads_for(s.T, ode_heads(s), s.C, s.S);
  const bool bwd = a.backward != 0;
  // loop-free form when every trajectory has its own workgroup (the grid policy is the caller's: ode_grid_for)
  const bool one = bwd && a.grid == s.B && !a.force_loop;
  const bool ra = bwd && s.grad_mode == SLODE_GRAD_REFERENCE_ADJOINT;
  // grid, block and LDS of a variant: PK trajectories with a map each, behind them the PK tanh rows [64] of ENCF (s_ehid) and the arrival
  // counters of SOFTB (s_sbar: one per trajectory, 16 slots)
  auto sized = [&](OdeVariant v) {
    const LdsMap m = ode_variant_map(v, s, npar, n_aux_lds, nthreads);
    v.ok = true; v.grid = a.grid / v.PK; v.nthreads = nthreads * v.PK; v.stn = m.stn;
    v.lds = sizeof(float) * ((size_t)v.PK * m.total + (v.ENCF ? (size_t)v.PK * 64 : 0) + (v.SOFTB ? 16 : 0));
    return v;
  };
  // ---- the form without the handle's arms: the scorer of an external solution, a named shape, or the generic kernel of its S
  int shape = s.H == ODE_H && s.S == 5 ? ODE_GENERIC5 : (s.H == ODE_H && s.S == 8 ? ODE_GENERIC8 : -1);
  bool scorer = false;
  if (a.x_ext && !a.force_generic) {
    bool aux16 = true;   // the scorer's cold-parameter path keeps a label head's weight row in 16 registers
    for (int q = 0; q < s.n_aux; ++q) aux16 = aux16 && s.aux[q].z_dim <= 16;
    scorer = a.alg == 0 && !ra && ode_dims_are(s, ODE_C2) && aux16 && s.method == SLODE_EULER && (!bwd || one);
    if (scorer) shape = ODE_C2;
  } else if (!a.force_generic) {
    for (int i = 0; i < ODE_N_NAMED; ++i) {
      if (!ode_shape_is(s, i)) continue;
      if (ode_cold_global(ode_shapes[i].L)) {
        // the cold parameter ranges [priors | W_1], W_z and the label heads are staged in the idle work block A | x | lam | st during P0
        // (COLDB): they must fit (they do for the reference's proc config: 4713 of 4768 floats); another split of the same dims may not,
        // and takes the generic kernel -- as do the measured arms' forward launches
        const LdsMap mc = ode_variant_map(ode_variant(i, ode_shapes[i], ODE_H, bwd, ra, one), s, npar, n_aux_lds, nthreads);
        const int ob = lay.ode_begin, o_b1 = lay.init_b1 - ob, n_aux = (a.with_ll && s.aux_in_main) ? s.n_aux : 0;
        const int cold = o_b1 + s.H * (1 + s.L) + (n_aux > 0 ? npar - (lay.aux_w1[0] - ob) : 0);
        if (a.alg != 0 || cold > 3 * mc.ax + mc.stn || o_b1 < 0) continue;
      }
      shape = i;
      break;
    }
  }
  OdeVariant v = ode_variant(shape, shape >= 0 ? ode_shapes[shape] : OdeShape{s.S, 0, 0, 0, 0, -1}, s.H, bwd, ra, one, scorer ? 3 : 0);
  if (scorer) v.M_ = SLODE_EULER;
  v = sized(v);
  if (v.lds > ODE_LDS_MAX) {
    snprintf(err, errlen, "ode kernel needs %zu B of LDS (> 160 KiB): T=%d S=%d too large", v.lds, s.T, s.S);
    return OdeVariant{};
  }
  const int cap = ode_max_threads(s.S, 0, 0, 0, one, bwd);   // the generic instantiation's declared block size
  if (nthreads > cap) {
    snprintf(err, errlen, "ode kernel: ode_state_dim %d with %s supports at most %d time points (got T=%d)", s.S,
             (one || !bwd) ? "one workgroup per trajectory" : "the persistent-loop grid (B > 65536)", cap, s.T);
    return OdeVariant{};
  }
  const bool metric = ode_shape_is(s, ODE_METRIC);
  const OdeShape& M = ode_shapes[ODE_METRIC];
  // measured A/B arms: direct evaluation of the dynamics heads, MFMA contraction -- metric shape, exact gradients, loop-free
  if (a.alg != 0 && bwd) {
    if (metric && one && !ra && !a.x_ext && (a.alg == 1 || a.alg == 2)) return sized(ode_variant(ODE_METRIC, M, ODE_H, true, false, true, a.alg));
    if (metric && one && !ra && !a.x_ext) snprintf(err, errlen, "unknown ode kernel variant %d", a.alg);
    else snprintf(err, errlen, "ode kernel variant %d is instantiated for the metric shape only (cvs T=200 L=8 rk4, exact gradients, B <= 65536)", a.alg);
    return OdeVariant{};
  }
  // fused encoder forward (metric shape, loop-free, folded encoder path): the caller skipped the enc_fwd2 launch
  if (a.enc_fuse) {
    if (!ode_takes_encf(s, bwd, a.grid, a.x_ext != nullptr, a.force_loop, a.force_generic, a.alg, a.pack)) {
      snprintf(err, errlen, "ode kernel: the fused encoder forward has no instantiation for this launch");
      return OdeVariant{};
    }
    // packed forms with the shared encoder pass and per-trajectory barriers (SOFTB): pack = 12 / 14 -> 2 / 4 trajectories per workgroup
    const int pk = a.pack == 14 ? 4 : (a.pack == 12 ? 2 : 1);
    const OdeVariant p = sized(ode_variant(ODE_METRIC, M, ODE_H, true, ra, true, 0, pk, true, pk > 1));
    return (pk == 1 || (s.B % pk == 0 && p.lds <= ODE_LDS_MAX)) ? p : sized(ode_variant(ODE_METRIC, M, ODE_H, true, ra, true, 0, 1, true));
  }
  // packed form: four trajectories per workgroup (metric shape, loop-free, batch a multiple of four)
  if (a.pack == 4 && one && a.alg == 0 && !a.x_ext && !a.force_generic && s.B % 4 == 0 && metric) {
    const OdeVariant p = sized(ode_variant(ODE_METRIC, M, ODE_H, true, ra, true, 0, 4));
    if (p.lds <= ODE_LDS_MAX) return p;
  }
  if (shape < 0) {
    snprintf(err, errlen, "ode kernel is instantiated for (ode_state_dim, ode_hidden_dim) in {(5,25),(8,25)}; got (%d,%d)", s.S, s.H);
    return OdeVariant{};
  }
  return v;
}

// ---- variant -> F<S, H, BWD, T_, C_, L_, Q_, M_, RA, ONE, ALG, PK, ENCF, SOFTB>::run(args...): every instantiation there is, named once
// (in the order the launcher has always named them: the order of the kernels in the object)
#define ODE_ARGS int, int, bool, int, int, int, int, int, bool, bool, int, int, bool, bool
template <template <ODE_ARGS> class F, int I, bool BWD, bool RA, bool ONE, int ALG = 0, int PK = 1, bool ENCF = false, bool SOFTB = false, int M_ = ode_shapes[I].method>
using OdeAt = F<ode_shapes[I].S, ODE_H, BWD, ode_shapes[I].T, ode_shapes[I].C, ode_shapes[I].L, ode_shapes[I].Q, M_, RA, ONE, ALG, PK, ENCF, SOFTB>;
// a backward form with exact gradients or the reference's adjoint (RA)
template <template <ODE_ARGS> class F, int I, bool ONE, int PK, bool ENCF, bool SOFTB, class... A>
auto ode_dispatch_bwd(bool ra, const A&... a) {
  return ra ? OdeAt<F, I, true, true, ONE, 0, PK, ENCF, SOFTB>::run(a...) : OdeAt<F, I, true, false, ONE, 0, PK, ENCF, SOFTB>::run(a...);
}
// the five forms every row of ode_shapes has: forward; backward loop-free (ONE) or looped, each exact or RA
template <template <ODE_ARGS> class F, int I, class... A>
auto ode_dispatch_shape(const OdeVariant& v, const A&... a) {
  if (!v.BWD) return OdeAt<F, I, false, false, false>::run(a...);
  return v.ONE ? ode_dispatch_bwd<F, I, true, 1, false, false>(v.RA, a...) : ode_dispatch_bwd<F, I, false, 1, false, false>(v.RA, a...);
}
template <template <ODE_ARGS> class F, class... A>
auto ode_dispatch(const OdeVariant& v, const A&... a) {
  if (v.ALG == 1) return OdeAt<F, ODE_METRIC, true, false, true, 1>::run(a...);
  if (v.ALG == 2) return OdeAt<F, ODE_METRIC, true, false, true, 2>::run(a...);
  if (v.SOFTB && v.PK == 4) return ode_dispatch_bwd<F, ODE_METRIC, true, 4, true, true>(v.RA, a...);
  if (v.SOFTB) return ode_dispatch_bwd<F, ODE_METRIC, true, 2, true, true>(v.RA, a...);
  if (v.ENCF) return ode_dispatch_bwd<F, ODE_METRIC, true, 1, true, false>(v.RA, a...);
  if (v.PK == 4) return ode_dispatch_bwd<F, ODE_METRIC, true, 4, false, false>(v.RA, a...);
  if (v.ALG == 3 && !v.BWD) return OdeAt<F, ODE_C2, false, false, false, 3, 1, false, false, SLODE_EULER>::run(a...);
  if (v.ALG == 3) return OdeAt<F, ODE_C2, true, false, true, 3, 1, false, false, SLODE_EULER>::run(a...);
  switch (v.shape) {
    case ODE_METRIC: return ode_dispatch_shape<F, ODE_METRIC>(v, a...);
    case ODE_C0: return ode_dispatch_shape<F, ODE_C0>(v, a...);
    case ODE_C2: return ode_dispatch_shape<F, ODE_C2>(v, a...);
    case ODE_C4: return ode_dispatch_shape<F, ODE_C4>(v, a...);
    case ODE_REF_DEFAULT: return ode_dispatch_shape<F, ODE_REF_DEFAULT>(v, a...);
    case ODE_GENERIC5: return ode_dispatch_shape<F, ODE_GENERIC5>(v, a...);
    default: return ode_dispatch_shape<F, ODE_GENERIC8>(v, a...);
  }
}
#undef ODE_ARGS

}  // namespace
